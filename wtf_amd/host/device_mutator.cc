// device_mutator.cc — --device-mutate for executors that do not mutate on the
// device (the oracle twin): the stream's one definition, csrc/engine_mutate.h,
// built for the host, over a host copy of the device corpus. The session
// materialises the same (index, ncorpus) orders the gpu backend hands to
// wtfgpu_mutate_feed_lanes, so a twin campaign is the reference for the flag.
#include "../csrc/engine_mutate.h"
#include "runner.h"

namespace wtfgpu_host {

bool DeviceCorpus::Add(const uint8_t *P, size_t N) {
  if (Count() >= MaxEntries || N > MaxBytes - Bytes.size()) return false;
  Bytes.insert(Bytes.end(), P, P + N);
  Off.push_back(Bytes.size());
  return true;
}

size_t DeviceMutate(uint64_t Seed, uint64_t Index, const DeviceCorpus &C, uint32_t NCorpus, uint32_t MaxLen,
                    uint8_t *Out) {
  return wtfmut::materialise(Seed, Index, wtfmut::Corpus{C.Bytes.data(), C.Off.data()}, NCorpus, MaxLen, Out);
}

}  // namespace wtfgpu_host
