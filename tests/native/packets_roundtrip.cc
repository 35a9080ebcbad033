// packets_roundtrip.cc — TEST INFRASTRUCTURE ONLY: the tlv module's
// PacketMutator_t conversions over a file of feeds, for
// tests/test_device_packets.py (linked with wtf_amd/host/libwtfhost.a).
//
//   packets_roundtrip <feeds>
// feeds: u32 length + bytes, repeated. For each feed f:
//   t = FeedToTestcase(f); TestcaseToFeed(t) must give f back; t must parse
//   (Deserialize) and Serialize of the parsed packets must be t.
// Prints "ok <count>" or the first failures.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../wtf_amd/host/wtf_api.h"

namespace TlvServer {  // as modules/fuzzer_tlv_server.cc defines them
struct Packet_t {
  uint32_t Command = 0;
  uint16_t Id = 0;
  uint16_t BodySize = 0;
  std::vector<uint8_t> Body;
};
bool Deserialize(const uint8_t *Buffer, const size_t BufferSize, std::vector<Packet_t> &Out);
std::string Serialize(const std::vector<Packet_t> &Packets);
}  // namespace TlvServer

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const Target_t *T = Targets_t::Instance().Get("tlv_server");
  if (!T || !T->PacketMutator) {
    puts("tlv_server declares no PacketMutator_t");
    return 1;
  }
  const PacketMutator_t &M = *T->PacketMutator;
  printf("params %u %u %u %u %u\n", M.GenMaxPackets, M.GenCommands, M.GenMaxBody, M.FlipOneIn, M.InsertMaxPackets);
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n;
  size_t count = 0, bad = 0;
  std::vector<uint8_t> feed, back;
  while (fread(&n, 4, 1, f) == 1) {
    feed.resize(n);
    if (n && fread(feed.data(), n, 1, f) != 1) return 2;
    const std::string t = M.FeedToTestcase(feed.data(), feed.size());
    const auto *tb = (const uint8_t *)t.data();
    std::vector<TlvServer::Packet_t> packets;
    const char *why = nullptr;
    if (!M.TestcaseToFeed(tb, t.size(), back)) why = "TestcaseToFeed refused";
    else if (back != feed) why = "TestcaseToFeed(FeedToTestcase(f)) != f";
    else if (!TlvServer::Deserialize(tb, t.size(), packets)) why = "Deserialize refused";
    else if (TlvServer::Serialize(packets) != t) why = "Serialize(Deserialize(t)) != t";
    if (why && bad++ < 5) printf("feed %zu (%u bytes): %s\n", count, n, why);
    count++;
  }
  fclose(f);
  if (bad) return 1;
  printf("ok %zu\n", count);
  return 0;
}
