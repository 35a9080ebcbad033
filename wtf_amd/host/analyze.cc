// analyze.cc — `analyze`: what each byte of one input does. The rule is
// csrc/engine_analyze.h's: every position of the input (a byte buffer's bytes;
// a feed's bytes without each chunk's four Size bytes) gets four candidates,
// the input with that one byte changed; each runs with full coverage, and the
// position's class comes from comparing the four outcomes (kind, crash name,
// the signature and size of the whole coverage set, overflow) with the
// input's own outcome and with each other.
//
// The input runs once as it is; its outcome is the base. An input whose own
// set overflowed is refused: nothing could be the same as it. The base goes
// to the device arena once. An executor with the device analyzer
// (GpuBackend_t) gets orders (entry, index) and makes the candidates in its
// lanes' feed regions; every other executor (the oracle twin), and the gpu one
// under WTFGPU_ANALYZE_HOST=1, gets the same candidates materialised here from
// the same header. An executor with the signature switch returns
// (sig, size, overflow) a candidate and no set; every other one, and the gpu
// one under WTFGPU_COVSIG_HOST=1, returns whole sets and the session computes
// the signature with the header's list form. A set of more than cap(--cov-set)
// values counts as overflowed there, which is when a lane's table of --cov-set
// slots drops a value.
//
// A candidate is a pure function of (input, index) and a class one of five
// outcomes, so the map depends on the input and the target alone, not on lane
// count, slice, lane order, queue, executor or either switch.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../csrc/engine_analyze.h"
#include "runner.h"

namespace wtfgpu_host {

namespace {

struct AnaSession {
  const RunnerOptions &O;
  Executor_t &Exec;
  Target_t &Target;
  ModuleSlots &Slots;
  bool Feeds = false;       // the feed stream (a PacketMutator_t target); else the byte stream
  bool Stream = false;      // candidates go through StreamStep; else RunBatch, Lanes() at a time
  bool OnDevice = false;    // the executor makes the candidates
  bool SigOnDevice = false; // the executor returns signatures
  PrepareInsert_t Prepare = nullptr;
  uint32_t CovCap = 0;
  uint64_t ReadbackValues = 0;

  // the base: its bytes (a feed's chunk bytes), and for a feed the indexed
  // entry the stream reads (wtfpkt::entry_write)
  std::vector<uint8_t> Base, Entry;
  uint32_t U = 0, DevEntry = 0;

  // the input's own run: these bytes as they are instead of a candidate
  const std::vector<uint8_t> *Literal = nullptr;

  std::map<std::string, uint32_t> Names;  // crash name -> id (from 1)
  std::vector<uint64_t> SetBuf;

  // one step's materialised candidates
  std::vector<uint8_t> Data, PrepData, Scratch, Buf;
  std::vector<uint64_t> Off, PrepOff;
  std::vector<PreparedInsert_t> Prep;

  // no LaneResult: the counted Ok_t without coverage, an empty set
  wtfana::Outcome OutcomeOf(const LaneResult *L) {
    wtfana::Outcome R{wtfana::kOk, 0, 0, 0, false};
    if (!L) return R;
    if (L->error) {
      R.kind = wtfana::kError;
    } else if (const Crash_t *C = std::get_if<Crash_t>(&L->result)) {
      R.kind = wtfana::kCrash;
      R.name = Names.emplace(C->CrashName, (uint32_t)Names.size() + 1).first->second;
    } else if (std::holds_alternative<Timedout_t>(L->result)) {
      R.kind = wtfana::kTimedout;
    } else if (std::holds_alternative<Cr3Change_t>(L->result)) {
      R.kind = wtfana::kCr3Change;
    }
    if (SigOnDevice && !Literal) {
      R.sig = L->cov_sig;
      R.size = L->cov_size;
      R.overflow = L->cov_overflow;
    } else {
      ReadbackValues += L->new_coverage.size();
      SetBuf = L->new_coverage;
      std::sort(SetBuf.begin(), SetBuf.end());
      SetBuf.erase(std::unique(SetBuf.begin(), SetBuf.end()), SetBuf.end());
      const wtfana::Sig S = wtfana::sig_list(SetBuf.data(), SetBuf.size());
      R.sig = S.sum;
      R.size = S.size;
      R.overflow = L->cov_overflow || SetBuf.size() > CovCap;
    }
    return R;
  }

  void SetBase(std::vector<uint8_t> B) {
    Base = std::move(B);
    U = (uint32_t)Base.size();
    if (Feeds) {
      const int64_t P = wtfpkt::entry_packets(Base.data(), Base.size(), kDevicePacketsMaxFeed);
      Entry.resize(wtfpkt::entry_bytes((uint64_t)P, Base.size()));
      wtfpkt::entry_write(Base.data(), Base.size(), (uint64_t)P, Entry.data());
    }
  }

  void Candidate(uint64_t Index, std::vector<uint8_t> &Out) const {
    Out.resize(Base.size());
    if (Feeds) wtfana::candidate_feed(Entry.data(), Index, Out.data());
    else wtfana::candidate_bytes(Base.data(), U, Index, Out.data());
  }

  // The step's testcases for the ordered candidates Idx[From, To)
  void Fill(const std::vector<uint64_t> &Idx, size_t From, size_t To, std::vector<StreamTestcase_t> &In) {
    In.clear();
    if (OnDevice && !Literal) {
      for (size_t i = From; i < To; i++) {
        StreamTestcase_t T{nullptr, 0, i};
        T.ordered = T.analyze = true;
        T.index = Idx[i];
        T.min_entry = DevEntry;
        In.push_back(T);
      }
      return;
    }
    Data.clear();
    PrepData.clear();
    Prep.clear();
    Off.assign(1, 0);
    PrepOff.assign(1, 0);
    for (size_t i = From; i < To; i++) {
      if (!Literal) Candidate(Idx[i], Buf);
      if (Literal) {
        Data.insert(Data.end(), Literal->begin(), Literal->end());
      } else if (Feeds) {  // the testcase the target makes of the feed
        const std::string Tc = Target.PacketMutator->FeedToTestcase(Buf.data(), Buf.size());
        Data.insert(Data.end(), Tc.begin(), Tc.end());
      } else {
        Data.insert(Data.end(), Buf.begin(), Buf.end());
      }
      Off.push_back(Data.size());
      if (Prepare) {
        Scratch.clear();
        const PreparedInsert_t K = Prepare(Data.data() + Off[Off.size() - 2], Data.size() - Off[Off.size() - 2], Scratch);
        Prep.push_back(K);
        if (K == PreparedInsert_t::Feed) PrepData.insert(PrepData.end(), Scratch.begin(), Scratch.end());
        PrepOff.push_back(PrepData.size());
      }
    }
    for (size_t i = From; i < To; i++) {
      const size_t k = i - From;
      StreamTestcase_t T{Data.data() + Off[k], (size_t)(Off[k + 1] - Off[k]), i};
      if (Prepare) {
        T.prep = Prep[k];
        T.prep_data = PrepData.data() + PrepOff[k];
        T.prep_size = (size_t)(PrepOff[k + 1] - PrepOff[k]);
      }
      In.push_back(T);
    }
  }

  // Runs the ordered candidates Idx; Done(i, outcome) as each finishes
  template <typename Fn> bool Run(const std::vector<uint64_t> &Idx, Fn &&Done) {
    const size_t N = Idx.size();
    std::vector<StreamTestcase_t> In;
    if (!Stream) {
      const size_t Lanes = std::max<uint32_t>(Exec.Lanes(), 1);
      std::vector<std::pair<const uint8_t *, size_t>> Tc;
      std::vector<LaneResult> R;
      for (size_t b = 0; b < N; b += Lanes) {
        const size_t e = std::min(N, b + Lanes);
        Fill(Idx, b, e, In);
        Tc.clear();
        for (const StreamTestcase_t &T : In) Tc.emplace_back(T.data, T.size);
        Exec.ResetCoverage();  // whole sets: every batch runs against an empty aggregate
        if (!Exec.RunBatch(Target, Tc, R, &Slots) || R.size() < e - b) return false;
        for (size_t i = b; i < e; i++) Done(i, OutcomeOf(&R[i - b]));
      }
      return true;
    }
    std::vector<StreamResult_t> R;
    size_t Next = 0, Got = 0;
    while (Got < N) {
      const size_t Want = std::min<size_t>(Exec.FreeLanes(), N - Next);
      Fill(Idx, Next, Next + Want, In);
      size_t Taken = 0;
      R.clear();
      if (!Exec.StreamStep(Target, In, O.slice, R, &Slots, &Taken)) return false;
      Next += Taken;  // the rest is offered again
      for (const StreamResult_t &F : R) {
        if (F.tag >= N) return false;
        Done((size_t)F.tag, OutcomeOf(F.r));
        Got++;
      }
    }
    return true;
  }
};

double SecondsSince(std::chrono::steady_clock::time_point T0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - T0).count();
}

std::string JsonEscape(const std::string &S) {
  std::string R;
  for (char c : S) {
    if (c == '"' || c == '\\') R += '\\';
    R += c;
  }
  return R;
}

const char *KindName(uint32_t Kind) {
  static const char *const N[] = {"ok", "crash", "timedout", "cr3", "error"};
  return Kind < wtfana::kNumKinds ? N[Kind] : "?";
}

// A feed position's place: its packet and the field it belongs to
const char *FieldOf(uint32_t InChunk) {
  return InChunk < 4 ? "size" : InChunk < 8 ? "command" : InChunk < 10 ? "id" : InChunk < 12 ? "bodysize" : "body";
}

}  // namespace

int AnalyzeMain(const RunnerOptions &O, Executor_t &Exec, Target_t &Target, ModuleSlots &Slots) {
  const auto T0 = std::chrono::steady_clock::now();
  AnaSession S{O, Exec, Target, Slots};
  S.CovCap = wtfkeep::cap(O.cov_set);
  // which stream the target gets
  const PacketMutator_t *M = Target.PacketMutator;
  const std::optional<InsertAction_t> &Ins = InsertAction_t::Declared();
  uint32_t MaxPayload = 0;
  if (M && M->FeedToTestcase && M->TestcaseToFeed) {
    S.Feeds = true;
  } else if (Ins) {
    MaxPayload = Ins->MaxPayload;
  } else {
    printf("analyze: target %s has neither a packet mutator (PacketMutator_t) nor a declared insert\n", O.name.c_str());
    return 1;
  }
  S.Stream = O.slice && Exec.CanStream();
  const fs::path InPath(O.input);
  if (!fs::is_regular_file(InPath)) {
    printf("analyze: --input %s is not a file\n", O.input.c_str());
    return 1;
  }
  const fs::path OutPath = O.output.empty() ? fs::path(O.input + ".map") : fs::path(O.output);
  {
    std::error_code Ec;
    if (fs::exists(OutPath, Ec)) {
      printf("analyze: --output %s exists (nothing is overwritten)\n", OutPath.string().c_str());
      return 1;
    }
  }
  const std::vector<uint8_t> Input = ReadFile(InPath);
  if (Input.empty()) {
    printf("analyze: %s has zero bytes: no position to analyze\n", O.input.c_str());
    return 1;
  }
  std::vector<uint8_t> First;
  if (S.Feeds) {
    if (!M->TestcaseToFeed(Input.data(), Input.size(), First) ||
        wtfpkt::entry_packets(First.data(), First.size(), kDevicePacketsMaxFeed) < 0) {
      printf("analyze: %s does not convert to a feed that fits a lane's feed region (%u bytes)\n", O.input.c_str(),
             kDevicePacketsMaxFeed);
      return 1;
    }
    if (First.empty()) {
      printf("analyze: %s is a feed of zero bytes: no position to analyze\n", O.input.c_str());
      return 1;
    }
  } else {
    if (Input.size() > kDeviceMutateMaxLen) {
      printf("analyze: %s is longer than a lane's feed region holds (%u bytes)\n", O.input.c_str(), kDeviceMutateMaxLen);
      return 1;
    }
    First = Input;
  }
  Exec.SetWantRegisters(false);
  if (S.Stream && Exec.TakesPrepared() && !Slots.Instances() && !getenv("WTF_NO_PREPARED_INSERT"))
    S.Prepare = Target.PrepareInsert;
  Exec.SetFullCoverage(true);  // whole sets: the input's and every candidate's

  // ---- the input, run once as it is: the base outcome
  wtfana::Outcome BaseOutcome{};
  {
    S.Literal = &Input;
    const bool Ran = S.Run(std::vector<uint64_t>{0}, [&](size_t, const wtfana::Outcome &R) { BaseOutcome = R; });
    S.Literal = nullptr;
    if (!Ran) {
      printf("analyze: the executor failed\n");
      return 1;
    }
    if (Exec.CoverageOverflowed() || BaseOutcome.overflow) {
      printf("analyze: the coverage set of %s filled up (a set of %u slots holds %u values), so no candidate could be "
             "the same as it; raise --cov-set\n", O.input.c_str(), O.cov_set, S.CovCap);
      return 1;
    }
  }
  std::string BaseName;
  for (const auto &[Name, Id] : S.Names)
    if (Id == BaseOutcome.name) BaseName = Name;

  const char *SigEnv = getenv("WTFGPU_COVSIG_HOST");
  if (Exec.HasDeviceCoverageSignature() && !(SigEnv && atoi(SigEnv) == 1)) {
    if (!Exec.SetCoverageSignature(true)) {
      printf("analyze: the executor refused the signature switch\n");
      return 1;
    }
    S.SigOnDevice = true;
  }
  S.SetBase(std::move(First));
  const char *HostEnv = getenv("WTFGPU_ANALYZE_HOST");
  const bool HostOnly = HostEnv && atoi(HostEnv) != 0;
  // (a byte buffer the module's InsertTestcase would reject, shorter than the
  // 4-byte head or longer than the head plus the declared insert's MaxPayload,
  // goes the host's way, where it is rejected as the input itself was)
  const bool Insertable = S.Feeds || (S.U >= 4 && !(MaxPayload && S.U > 4ull + MaxPayload));
  if (Exec.HasDeviceAnalyzer() && S.Stream && !HostOnly && Insertable) {
    if (!Exec.SetDeviceAnalyze(S.Feeds)) {
      printf("analyze: the executor does not put target %s's candidates into the guest on the device\n",
             O.name.c_str());
      return 1;
    }
    if (!Exec.DeviceAnalyzeBase(S.Base.data(), S.Base.size(), &S.DevEntry)) {  // the base goes up once
      printf("analyze: the device arena refused the base\n");
      return 1;
    }
    S.OnDevice = true;
  }

  // ---- the positions, and every candidate of every one that is not framing
  std::string Classes(S.U, (char)wtfana::kFraming);
  std::vector<uint32_t> Packet(S.U, 0), InChunk(S.U, 0);  // feeds: each position's chunk and offset in it
  std::vector<uint64_t> Idx;
  if (S.Feeds) {
    const uint32_t P = wtfpkt::ld32(S.Entry.data());
    std::vector<uint32_t> Coff(P + 1);
    memcpy(Coff.data(), S.Entry.data() + 4, Coff.size() * 4);
    for (uint32_t k = 0; k < P; k++)
      for (uint32_t p = Coff[k]; p < Coff[k + 1]; p++) Packet[p] = k, InChunk[p] = p - Coff[k];
    for (uint32_t p = 0; p < S.U; p++)
      if (!wtfana::is_framing(Coff.data(), P, p))
        for (uint32_t v = 0; v < wtfana::kVariants; v++) Idx.push_back(4ull * p + v);
  } else {
    for (uint64_t I = 0; I < wtfana::total(S.U); I++) Idx.push_back(I);
  }
  const uint64_t Positions = Idx.size() / wtfana::kVariants;
  uint64_t Count[5] = {0, 0, 0, 0, 0}, Overflowed = 0;  // . m F V #
  Count[4] = S.U - Positions;
  std::vector<wtfana::Outcome> Got(Idx.size());
  std::vector<uint8_t> In(Positions, 0);  // outcomes in, a position (Idx holds a position's four in a row)
  const bool Ran = S.Run(Idx, [&](size_t i, const wtfana::Outcome &R) {
    Got[i] = R;
    Overflowed += R.overflow;
    const size_t q = i / wtfana::kVariants;
    if (++In[q] < wtfana::kVariants) return;
    const char C = wtfana::classify(BaseOutcome, &Got[q * wtfana::kVariants]);
    Classes[(size_t)(Idx[i] >> 2)] = C;
    Count[C == wtfana::kNone ? 0 : C == wtfana::kMinor ? 1 : C == wtfana::kFixed ? 2 : 3]++;
  });
  if (!Ran) {
    printf("analyze: the executor failed\n");
    return 1;
  }
  if (S.SigOnDevice) Exec.SetCoverageSignature(false);

  // ---- the map
  std::string J = "{\"bytes\":" + std::to_string(S.U) + ",\"base\":{\"kind\":\"" + KindName(BaseOutcome.kind) +
                  "\",\"crash\":\"" + JsonEscape(BaseName) + "\",\"values\":" + std::to_string(BaseOutcome.size) +
                  "},\"classes\":\"" + Classes + "\",\"ranges\":[";
  bool FirstRange = true;
  for (uint32_t lo = 0; lo < S.U;) {
    uint32_t hi = lo + 1;
    const auto Joins = [&](uint32_t p) {
      return Classes[p] == Classes[lo] &&
             (!S.Feeds || (Packet[p] == Packet[lo] && !strcmp(FieldOf(InChunk[p]), FieldOf(InChunk[lo]))));
    };
    while (hi < S.U && Joins(hi)) hi++;
    J += std::string(FirstRange ? "" : ",") + "{\"lo\":" + std::to_string(lo) + ",\"hi\":" + std::to_string(hi) +
         ",\"class\":\"" + Classes[lo] + "\"";
    if (S.Feeds) J += ",\"packet\":" + std::to_string(Packet[lo]) + ",\"field\":\"" + FieldOf(InChunk[lo]) + "\"";
    J += "}";
    FirstRange = false;
    lo = hi;
  }
  J += "]}\n";
  if (!SaveFile(OutPath, (const uint8_t *)J.data(), J.size())) {
    printf("analyze: could not write %s\n", OutPath.string().c_str());
    return 1;
  }
  printf("{\"mode\":\"analyze\",\"bytes\":%u,\"positions\":%llu,\"candidates\":%zu,\"none\":%llu,\"minor\":%llu,"
         "\"fixed\":%llu,\"variable\":%llu,\"framing\":%llu,\"overflowed\":%llu,\"on_device\":%s,\"sig_on_device\":%s,"
         "\"sig_readback_values\":%llu,\"executor\":%s,\"seconds\":%.3f}\n",
         S.U, (unsigned long long)Positions, Idx.size(), (unsigned long long)Count[0], (unsigned long long)Count[1],
         (unsigned long long)Count[2], (unsigned long long)Count[3], (unsigned long long)Count[4],
         (unsigned long long)Overflowed, S.OnDevice ? "true" : "false", S.SigOnDevice ? "true" : "false",
         (unsigned long long)S.ReadbackValues, Exec.StatsJson().c_str(), SecondsSince(T0));
  return 0;
}

}  // namespace wtfgpu_host
