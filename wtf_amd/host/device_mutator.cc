// device_mutator.cc — --device-mutate for executors that do not mutate on the
// device (the oracle twin): the stream's one definition, csrc/engine_mutate.h,
// built for the host, over a host copy of the device corpus. The session
// materialises the same (index, ncorpus) orders the gpu backend hands to
// wtfgpu_mutate_feed_lanes, so a twin campaign is the reference for the flag.
#include "../csrc/engine_mutate.h"
#include "../csrc/engine_mutate_packets.h"
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

// ---- --device-packets: csrc/engine_mutate_packets.h, the same way

bool DeviceCorpus::AddFeed(const uint8_t *Feed, size_t N) {
  const int64_t P = wtfpkt::entry_packets(Feed, N, kDevicePacketsMaxFeed);
  if (P < 0) return false;
  const uint64_t E = wtfpkt::entry_bytes((uint64_t)P, N);
  if (Count() >= MaxEntries || E > MaxBytes - Bytes.size()) return false;
  const size_t At = Bytes.size();
  Bytes.resize(At + E);
  wtfpkt::entry_write(Feed, N, (uint64_t)P, Bytes.data() + At);
  Off.push_back(Bytes.size());
  return true;
}

static wtfpkt::Params PacketParams(const PacketMutator_t &M) {
  return wtfpkt::Params{M.GenMaxPackets, M.GenCommands,      M.GenMaxBody,
                        M.FlipOneIn,     M.InsertMaxPackets, kDevicePacketsMaxFeed};
}

bool DevicePacketsParamsValid(const PacketMutator_t &M) { return wtfpkt::params_valid(PacketParams(M)); }

size_t DevicePackets(uint64_t Seed, uint64_t Index, const DeviceCorpus &C, uint32_t NCorpus, const PacketMutator_t &M,
                     uint8_t *Out) {
  return wtfpkt::materialise(Seed, Index, wtfpkt::Corpus{C.Bytes.data(), C.Off.data()}, NCorpus, PacketParams(M), Out);
}

}  // namespace wtfgpu_host
