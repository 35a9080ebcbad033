// sim_packets.cc — TEST INFRASTRUCTURE ONLY: the device packet mutator's
// definition (wtf_amd/csrc/engine_mutate_packets.h) built for the host, behind
// a C interface for tests/test_device_packets.py.
#include <cstring>

#include "../../wtf_amd/csrc/engine_mutate_packets.h"

extern "C" {

// Testcase indices[i] of the stream, i < n, over the first ncorpus entries of
// an arena in the indexed layout, into out + i * stride (stride >= params[5],
// MaxFeed); lens[i] its size; info[2 * i ..] what it was (wtfpkt::What) and,
// generated, its packets. params: GenMaxPackets, GenCommands, GenMaxBody,
// FlipOneIn, InsertMaxPackets, MaxFeed.
void sim_packets_many(uint64_t seed, const uint64_t *indices, uint32_t n, const uint8_t *bytes, const uint64_t *off,
                      uint32_t ncorpus, const uint32_t *params, uint8_t *out, uint64_t stride, uint32_t *lens,
                      uint32_t *info) {
  const wtfpkt::Corpus c{bytes, off};
  const wtfpkt::Params q{params[0], params[1], params[2], params[3], params[4], params[5]};
  for (uint32_t i = 0; i < n; i++) {
    wtfpkt::Info what;
    lens[i] = wtfpkt::materialise(seed, indices[i], c, ncorpus, q, out + i * stride, &what);
    if (info) {
      info[2 * i] = what.what;
      info[2 * i + 1] = what.packets;
    }
  }
}

int sim_packets_params_valid(const uint32_t *params) {
  return wtfpkt::params_valid(wtfpkt::Params{params[0], params[1], params[2], params[3], params[4], params[5]});
}

// The gate of wtfgpu_corpus_add_feed: packets of a feed (-1: refused), and its
// entry in the indexed layout (entry must hold sim_packets_entry_bytes bytes).
int64_t sim_packets_entry_packets(const uint8_t *feed, uint64_t len, uint32_t max_feed) {
  return wtfpkt::entry_packets(feed, len, max_feed);
}
uint64_t sim_packets_entry_bytes(uint64_t packets, uint64_t len) { return wtfpkt::entry_bytes(packets, len); }
void sim_packets_entry_write(const uint8_t *feed, uint64_t len, uint64_t packets, uint8_t *entry) {
  wtfpkt::entry_write(feed, len, packets, entry);
}
}
