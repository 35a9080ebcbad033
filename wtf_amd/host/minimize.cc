// minimize.cc — `minimize`: shrink one crashing testcase, keeping its crash
// name. The candidates are the stream of csrc/engine_minimize.h (levels of
// halving chunks; REMOVE, then ZERO for byte buffers): an executor with the
// device minimiser (GpuBackend_t) gets orders (entry, op, index) and makes the
// candidates in its lanes' feed regions; every other executor (the oracle
// twin), and the gpu one under WTFGPU_MINIMIZE_HOST=1, gets the same candidates
// materialised here from the same header, through the ordinary upload path. No
// candidate is read back: the winner is re-derived here.
//
// A round is every candidate of the current base under the current op, minus
// the ones never ordered (`skipped`): what the module's InsertTestcase would
// reject (byte stream: shorter than the 4-byte head, longer than the head plus
// the declared insert's MaxPayload) and ZERO candidates whose range holds no
// non-zero byte. Nothing is selected before every ordered candidate has a
// result. A candidate matches iff its result is a Crash_t of the input's name.
// REMOVE: the smallest matching result wins; ZERO: the one that zeroes the
// most non-zero bytes; ties go to the lowest index. The winner is the next
// round's base. REMOVE rounds run until one has no match, then ZERO rounds
// likewise; so the result depends on the input and the target alone, not on
// lane count, slice, lane order, queue or executor.
//
// --keep-coverage: the same session for an input that ends Ok_t, with another
// match rule, the one of csrc/engine_covkeep.h. The input's own run happens
// with full coverage; its whole set, sorted and unique, is the target T for
// the whole session. A candidate matches iff it ends Ok_t without an engine
// error, its set did not overflow and lacks none of T's values. An executor
// with the device check (GpuBackend_t) is given T once and returns a verdict a
// candidate, no set; every other executor (the oracle twin), and the gpu one
// under WTFGPU_COVKEEP_HOST=1, stays in full coverage and the session counts
// the missing values of each candidate's new_coverage with the header's host
// function. A set of more than cap(--cov-set) values counts as overflowed
// there, which is when a lane's table of --cov-set slots drops a value.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/engine_covkeep.h"
#include "../csrc/engine_minimize.h"
#include "runner.h"

namespace wtfgpu_host {

namespace {

struct MinSession {
  const RunnerOptions &O;
  Executor_t &Exec;
  Target_t &Target;
  ModuleSlots &Slots;
  bool Feeds = false;     // the feed stream (a PacketMutator_t target); else the byte stream
  bool Stream = false;    // rounds go through StreamStep; else RunBatch, Lanes() at a time
  bool OnDevice = false;  // the executor makes the candidates
  PrepareInsert_t Prepare = nullptr;
  uint32_t MaxPayload = 0;
  std::string W;  // the crash name to keep

  // --keep-coverage: the target set instead of a crash name; the executor
  // holds it and returns verdicts (CovOnDevice) or the session checks sets of
  // at most CovCap values itself
  bool KeepCov = false, CovOnDevice = false;
  std::vector<uint64_t> T;
  uint32_t CovCap = 0;
  // candidates that ended Ok_t without an error but lacked a value of T, or
  // whose set overflowed; coverage values handed to the session
  uint64_t OkButMissing = 0, Overflowed = 0, ReadbackValues = 0;
  std::vector<uint64_t> SetBuf;

  // the current base: its bytes (a feed's chunk bytes), its units, and for a
  // feed the indexed entry the stream reads (wtfpkt::entry_write)
  std::vector<uint8_t> Base, Entry;
  uint32_t U = 0, DevEntry = 0;
  uint32_t Op = wtfmin::kRemove;

  // the input's own run, before any candidate: these bytes as they are
  // instead of a candidate, and the result kept
  const std::vector<uint8_t> *Literal = nullptr;
  LaneResult LiteralResult;

  // one step's materialised candidates
  std::vector<uint8_t> Data, PrepData, Scratch, Buf;
  std::vector<uint64_t> Off, PrepOff;
  std::vector<PreparedInsert_t> Prep;

  // *Values: the entries of the candidate's coverage set (--keep-coverage)
  bool Matches(const LaneResult *L, uint32_t *Values) {
    *Values = 0;
    if (!KeepCov) {
      if (!L || L->error) return false;
      const Crash_t *C = std::get_if<Crash_t>(&L->result);
      return C && C->CrashName == W;
    }
    if (L) ReadbackValues += L->new_coverage.size();
    if (Literal) return false;  // the input's own run: MinimizeMain reads LiteralResult
    // no LaneResult: the counted Ok_t without coverage, an empty set (an
    // executor with a target set never returns it)
    bool Ok = true, Error = false, Ovf = false;
    uint64_t Missing = T.size();
    if (L) {
      Ok = std::holds_alternative<Ok_t>(L->result);
      Error = L->error;
      if (CovOnDevice) {
        Missing = L->cov_missing;
        Ovf = L->cov_overflow;
        *Values = L->cov_size;
      } else {
        SetBuf = L->new_coverage;
        std::sort(SetBuf.begin(), SetBuf.end());
        SetBuf.erase(std::unique(SetBuf.begin(), SetBuf.end()), SetBuf.end());
        Missing = wtfkeep::missing_sorted(SetBuf.data(), SetBuf.size(), T.data(), T.size());
        Ovf = L->cov_overflow || SetBuf.size() > CovCap;
        *Values = (uint32_t)SetBuf.size();
      }
    }
    if (Ok && !Error) {
      if (Ovf) Overflowed++;
      else if (Missing) OkButMissing++;
    }
    return wtfkeep::keeps(Ok, Error, Ovf, Missing);
  }

  void SetBase(std::vector<uint8_t> B) {
    Base = std::move(B);
    if (Feeds) {
      const int64_t P = wtfpkt::entry_packets(Base.data(), Base.size(), kDevicePacketsMaxFeed);
      U = (uint32_t)P;  // a candidate of a valid feed is a valid feed
      Entry.resize(wtfpkt::entry_bytes((uint64_t)P, Base.size()));
      wtfpkt::entry_write(Base.data(), Base.size(), (uint64_t)P, Entry.data());
    } else {
      U = (uint32_t)Base.size();
    }
  }

  // candidate Index of the current op into Out; its size
  uint32_t Candidate(uint64_t Index, std::vector<uint8_t> &Out) const {
    Out.resize(Base.size() + 1);
    const uint32_t N = Feeds ? wtfmin::candidate_feed(Entry.data(), Index, Out.data())
                             : wtfmin::candidate_bytes(Base.data(), U, Op, Index, Out.data());
    Out.resize(N);
    return N;
  }

  // Size of the candidate's result in bytes, and for ZERO the non-zero bytes it clears
  void Measure(uint64_t Index, uint32_t &Size, uint32_t &Cleared) const {
    wtfmin::Plan P;
    if (Feeds) wtfmin::plan_feed(P, Entry.data(), Index);
    else wtfmin::plan_bytes(P, Base.data(), U, Op, Index);
    Size = P.size;
    Cleared = 0;
    for (uint32_t k = 0; k < P.n; k++) Cleared += Base[P.a + k] != 0;
  }

  bool Skipped(uint32_t Size, uint32_t Cleared) const {
    if (Op == wtfmin::kZero && Cleared == 0) return true;
    if (Feeds) return false;
    return Size < 4 || (MaxPayload && Size > 4ull + MaxPayload);
  }

  // The step's testcases for the round's ordered candidates Idx[From, To)
  void Fill(const std::vector<uint64_t> &Idx, size_t From, size_t To, std::vector<StreamTestcase_t> &In) {
    In.clear();
    if (OnDevice) {
      for (size_t i = From; i < To; i++) {
        StreamTestcase_t T{nullptr, 0, i};
        T.ordered = T.minimize = true;
        T.index = Idx[i];
        T.min_entry = DevEntry;
        T.min_op = Op;
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

  // Runs the ordered candidates Idx; Match[i] = candidate Idx[i] keeps the
  // crash (--keep-coverage: the coverage, and Values[i] = its set's entries)
  bool RunRound(const std::vector<uint64_t> &Idx, std::vector<uint8_t> &Match, std::vector<uint32_t> &Values) {
    const size_t N = Idx.size();
    Match.assign(N, 0);
    Values.assign(N, 0);
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
        if (KeepCov) Exec.ResetCoverage();  // whole sets: every batch runs against an empty aggregate
        if (!Exec.RunBatch(Target, Tc, R, &Slots) || R.size() < e - b) return false;
        for (size_t i = b; i < e; i++) Match[i] = Matches(&R[i - b], &Values[i]);
        if (Literal && !R.empty()) LiteralResult = R[0];
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
        Match[F.tag] = Matches(F.r, &Values[F.tag]);
        if (Literal) LiteralResult = F.r ? *F.r : LaneResult{};  // (no LaneResult: the common Ok_t)
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

}  // namespace

int MinimizeMain(const RunnerOptions &O, Executor_t &Exec, Target_t &Target, ModuleSlots &Slots) {
  const auto T0 = std::chrono::steady_clock::now();
  MinSession S{O, Exec, Target, Slots};
  S.KeepCov = O.keep_coverage;
  S.CovCap = wtfkeep::cap(O.cov_set);
  // which stream the target gets
  const PacketMutator_t *M = Target.PacketMutator;
  const std::optional<InsertAction_t> &Ins = InsertAction_t::Declared();
  if (M && M->FeedToTestcase && M->TestcaseToFeed) {
    S.Feeds = true;
  } else if (Ins && Target.CreateMutator == LibfuzzerMutator_t::Create) {
    S.MaxPayload = Ins->MaxPayload;
  } else {
    printf("minimize: target %s has neither a packet mutator (PacketMutator_t) nor a declared insert with the default "
           "mutator\n", O.name.c_str());
    return 1;
  }
  S.Stream = O.slice && Exec.CanStream();
  if (Exec.HasDeviceMinimizer() && !S.Stream) {
    printf("minimize needs a streaming run on this executor (--slice-steps != 0)\n");
    return 1;
  }
  const fs::path InPath(O.input);
  if (!fs::is_regular_file(InPath)) {
    printf("minimize: --input %s is not a file\n", O.input.c_str());
    return 1;
  }
  const std::vector<uint8_t> Input = ReadFile(InPath);
  std::vector<uint8_t> First;
  if (S.Feeds) {
    if (!M->TestcaseToFeed(Input.data(), Input.size(), First) ||
        wtfpkt::entry_packets(First.data(), First.size(), kDevicePacketsMaxFeed) < 0) {
      printf("minimize: %s does not convert to a feed that fits a lane's region\n", O.input.c_str());
      return 1;
    }
  } else {
    First = Input;
  }
  Exec.SetWantRegisters(false);
  if (S.Stream && Exec.TakesPrepared() && !Slots.Instances() && !getenv("WTF_NO_PREPARED_INSERT"))
    S.Prepare = Target.PrepareInsert;

  // whole sets: the input's, and without the device check every candidate's
  if (S.KeepCov) Exec.SetFullCoverage(true);
  // ---- the input, run once as it is: its crash name is the one to keep
  // (--keep-coverage: its whole coverage set)
  std::vector<uint8_t> Match;
  std::vector<uint32_t> Values;
  {
    S.Literal = &Input;
    const bool Ran = S.RunRound(std::vector<uint64_t>{0}, Match, Values);
    S.Literal = nullptr;
    if (!Ran) {
      printf("minimize: the executor failed\n");
      return 1;
    }
    const LaneResult &R = S.LiteralResult;
    const Crash_t *C = std::get_if<Crash_t>(&R.result);
    if (S.KeepCov) {
      if (!R.error && C) {
        printf("minimize: %s crashes (%s): drop --keep-coverage to minimise it by its crash name\n", O.input.c_str(),
               C->CrashName.c_str());
        return 1;
      }
      if (R.error || !std::holds_alternative<Ok_t>(R.result)) {
        printf("minimize: %s does not end ok (%s): --keep-coverage minimises a testcase that does\n", O.input.c_str(),
               R.error ? "engine error" : TestcaseResultName(R.result).c_str());
        return 1;
      }
      S.T = R.new_coverage;
      std::sort(S.T.begin(), S.T.end());
      S.T.erase(std::unique(S.T.begin(), S.T.end()), S.T.end());
      if (Exec.CoverageOverflowed() || R.cov_overflow || S.T.size() > S.CovCap) {
        printf("minimize: the coverage set of %s filled up (a set of %u slots holds %u values), so the target would be "
               "incomplete; raise --cov-set\n", O.input.c_str(), O.cov_set, S.CovCap);
        return 1;
      }
    } else if (R.error || !C || C->CrashName.empty()) {
      printf("minimize: %s does not crash (%s): nothing to minimise\n", O.input.c_str(),
             R.error ? "engine error" : TestcaseResultName(R.result).c_str());
      return 1;
    }
    if (!S.KeepCov) S.W = C->CrashName;
  }
  if (S.KeepCov) {
    const char *CovEnv = getenv("WTFGPU_COVKEEP_HOST");
    if (Exec.HasDeviceCoverageCheck() && !(CovEnv && atoi(CovEnv) == 1)) {
      if (!Exec.SetCoverageTarget(S.T.data(), S.T.size())) {
        printf("minimize: the executor refused the coverage target\n");
        return 1;
      }
      S.CovOnDevice = true;
    }
  }
  const char *HostEnv = getenv("WTFGPU_MINIMIZE_HOST");
  const bool HostOnly = HostEnv && atoi(HostEnv) != 0;
  // (a byte buffer longer than a feed region's chunk cannot be a device base:
  // such an input's candidates are uploaded)
  if (Exec.HasDeviceMinimizer() && !HostOnly && (S.Feeds || First.size() <= kDeviceMutateMaxLen)) {
    if (!Exec.SetDeviceMinimize(S.Feeds)) {
      printf("minimize: the executor does not put target %s's candidates into the guest on the device\n",
             O.name.c_str());
      return 1;
    }
    S.OnDevice = true;
  }

  uint64_t Rounds = 0, RemoveRounds = 0, ZeroRounds = 0, Candidates = 0, SkippedN = 0, UploadBytes = 0;
  bool StoppedByRounds = false;
  S.SetBase(std::move(First));
  std::vector<uint64_t> Idx;
  std::vector<uint32_t> Size, Cleared;
  uint64_t OutputValues = S.T.size();
  for (S.Op = wtfmin::kRemove; S.Op < (S.Feeds ? wtfmin::kZero : wtfmin::kNumOps);) {
    if (Rounds >= O.rounds) {
      StoppedByRounds = true;
      break;
    }
    Rounds++;
    (S.Op == wtfmin::kRemove ? RemoveRounds : ZeroRounds)++;
    const uint64_t T = wtfmin::total(S.U);
    Idx.clear();
    Size.clear();
    Cleared.clear();
    for (uint64_t I = 0; I < T; I++) {
      uint32_t Sz, Cl;
      S.Measure(I, Sz, Cl);
      if (S.Skipped(Sz, Cl)) {
        SkippedN++;
        continue;
      }
      Idx.push_back(I);
      Size.push_back(Sz);
      Cleared.push_back(Cl);
      if (!S.OnDevice) UploadBytes += Sz;
    }
    Candidates += Idx.size();
    if (S.OnDevice && !Idx.empty()) {  // the base goes up once a round
      if (!Exec.DeviceMinimizeBase(S.Base.data(), S.Base.size(), &S.DevEntry)) {
        printf("minimize: the device arena refused the base\n");
        return 1;
      }
      UploadBytes += S.Base.size();
    }
    if (!S.RunRound(Idx, Match, Values)) {
      printf("minimize: the executor failed\n");
      return 1;
    }
    size_t Best = Idx.size();
    for (size_t i = 0; i < Idx.size(); i++) {
      if (!Match[i]) continue;
      if (Best == Idx.size() || (S.Op == wtfmin::kRemove ? Size[i] < Size[Best] : Cleared[i] > Cleared[Best])) Best = i;
    }
    if (Best == Idx.size()) {  // no match: the phase is over
      S.Op++;
      continue;
    }
    OutputValues = Values[Best];
    std::vector<uint8_t> Next;
    S.Candidate(Idx[Best], Next);
    S.SetBase(std::move(Next));
  }

  std::string Out;
  if (S.Feeds) Out = M->FeedToTestcase(S.Base.data(), S.Base.size());
  else Out.assign(S.Base.begin(), S.Base.end());
  const fs::path OutPath = O.output.empty() ? fs::path(O.input + ".min") : fs::path(O.output);
  if (!SaveFile(OutPath, (const uint8_t *)Out.data(), Out.size())) {
    printf("minimize: could not write %s\n", OutPath.string().c_str());
    return 1;
  }
  if (S.CovOnDevice) Exec.ClearCoverageTarget();
  char Cov[256] = "";
  if (S.KeepCov)
    snprintf(Cov, sizeof(Cov), "\"values\":%zu,\"output_values\":%llu,\"cov_on_device\":%s,"
             "\"cov_readback_values\":%llu,\"overflowed\":%llu,\"ok_but_missing\":%llu,", S.T.size(), (unsigned long long)OutputValues,
             S.CovOnDevice ? "true" : "false", (unsigned long long)S.ReadbackValues, (unsigned long long)S.Overflowed,
             (unsigned long long)S.OkButMissing);
  printf("{\"mode\":\"%s\",%s\"input_bytes\":%zu,\"output_bytes\":%zu,\"rounds\":%llu,\"remove_rounds\":%llu,"
         "\"zero_rounds\":%llu,\"candidates\":%llu,\"skipped\":%llu,\"crash\":\"%s\",\"stopped_by_rounds\":%s,\"seconds\":%.3f,"
         "\"on_device\":%s,\"upload_bytes\":%llu,\"executor\":%s}\n",
         S.KeepCov ? "coverage" : "crash", Cov, Input.size(), Out.size(), (unsigned long long)Rounds,
         (unsigned long long)RemoveRounds, (unsigned long long)ZeroRounds, (unsigned long long)Candidates, (unsigned long long)SkippedN,
         JsonEscape(S.W).c_str(), StoppedByRounds ? "true" : "false", SecondsSince(T0), S.OnDevice ? "true" : "false",
         (unsigned long long)UploadBytes, Exec.StatsJson().c_str());
  return 0;
}

}  // namespace wtfgpu_host
