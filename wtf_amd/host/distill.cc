// distill.cc — `distill`: cut a corpus to a covering subset. Every input is
// replayed once for its whole coverage set (parity mode, the way `run`'s
// streaming replay reads them), the inputs are ranked by (file size, file
// name), and the greedy cover of csrc/engine_distill.h picks the subset: in
// every round the input that adds the most values not yet covered, the
// smaller file among equals. An executor with the device distiller
// (GpuBackend_t: wtfgpu_distill) runs the cover on the device; every other
// executor (the oracle twin), and the gpu one under WTFGPU_DISTILL_HOST=1,
// runs distill_host from the same header.
//
// Eligible inputs are those that end Ok_t with no engine error: a crash, a
// timeout (which commits no coverage in the reference either,
// client.cc:120-126), a cr3 change, an engine error or a failed insert is
// excluded and counted by kind. The sets depend on the input and the target
// alone, so the kept files do not depend on lane count, slice, queue,
// --device-attrib or executor.
//
// Nothing is written before every check has passed: the kept files are copied
// under their own names into --output (which must be missing or an empty
// directory; nothing is ever deleted), then --results gets one JSON line per
// input in rank order, and the last stdout line is the summary.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/engine_distill.h"
#include "runner.h"

namespace wtfgpu_host {

namespace {

struct DistillInput {
  fs::path path;
  std::string name;
  uint64_t bytes = 0;
  std::string result;             // TestcaseResultName, or "error"
  bool eligible = false;
  std::vector<uint64_t> values;   // the whole coverage set, sorted and unique
  int64_t order = -1;             // its place among the taken (-1: not kept)
  uint32_t gain = 0;
};

double MsSince(std::chrono::steady_clock::time_point T0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
}

std::string Escape(const std::string &S) {
  std::string R;
  for (char c : S) {
    if (c == '"' || c == '\\') R += '\\';
    R += c;
  }
  return R;
}

struct Excluded {
  uint64_t crash = 0, timeout = 0, cr3 = 0, error = 0, insert_failed = 0;
};

// One input's result into its record, counted by kind
void Classify(DistillInput &In, const LaneResult *L, Excluded &X) {
  if (!L) {  // the common counted result: Ok_t, no error, no coverage
    In.result = "ok";
    In.eligible = true;
    return;
  }
  In.result = L->error ? "error" : TestcaseResultName(L->result);
  In.values = L->new_coverage;
  std::sort(In.values.begin(), In.values.end());
  In.values.erase(std::unique(In.values.begin(), In.values.end()), In.values.end());
  if (L->error) {
    X.error++;
  } else if (const Crash_t *C = std::get_if<Crash_t>(&L->result)) {
    (C->CrashName == "insert-testcase-failed" ? X.insert_failed : X.crash)++;
  } else if (std::holds_alternative<Timedout_t>(L->result)) {
    X.timeout++;
  } else if (std::holds_alternative<Cr3Change_t>(L->result)) {
    X.cr3++;
  } else {
    In.eligible = true;
  }
}

}  // namespace

int DistillMain(const RunnerOptions &O, Executor_t &Exec, Target_t &Target, ModuleSlots &Slots) {
  const auto T0 = std::chrono::steady_clock::now();
  // ---- the refusals that need no run
  const fs::path OutDir(O.output);
  std::error_code Ec;
  if (fs::exists(OutDir, Ec) && (!fs::is_directory(OutDir, Ec) || !fs::is_empty(OutDir, Ec))) {
    printf("distill: --output %s exists and is not an empty directory (nothing is overwritten or deleted)\n",
           O.output.c_str());
    return 1;
  }
  const fs::path InDir = O.input.empty() ? fs::path(O.target) / "inputs" : fs::path(O.input);
  std::vector<DistillInput> In;
  if (fs::is_directory(InDir, Ec)) {
    for (const auto &E : fs::directory_iterator(InDir))
      if (E.is_regular_file()) In.push_back(DistillInput{E.path(), E.path().filename().string(), E.file_size()});
  } else if (fs::is_regular_file(InDir, Ec)) {
    In.push_back(DistillInput{InDir, InDir.filename().string(), fs::file_size(InDir)});
  }
  if (In.empty()) {
    printf("distill: no inputs in %s\n", InDir.string().c_str());
    return 1;
  }
  // rank order: the smaller file first, then the name
  std::sort(In.begin(), In.end(), [](const DistillInput &A, const DistillInput &B) {
    return A.bytes != B.bytes ? A.bytes < B.bytes : A.name < B.name;
  });

  // ---- the replay: every input once, whole sets
  const size_t N = In.size();
  Exec.SetFullCoverage(true);
  Exec.SetWantRegisters(false);
  Excluded X;
  const bool Stream = O.slice && Exec.CanStream();
  if (Stream) {
    std::vector<std::vector<uint8_t>> Bufs(N);
    std::vector<StreamTestcase_t> Step;
    std::vector<StreamResult_t> R;
    size_t Next = 0, Got = 0;
    while (Got < N) {
      Step.clear();
      for (uint32_t F = Exec.FreeLanes(); F && Next < N; F--, Next++) {
        Bufs[Next] = ReadFile(In[Next].path);
        Step.push_back(StreamTestcase_t{Bufs[Next].data(), Bufs[Next].size(), Next});
      }
      size_t Taken = 0;
      R.clear();
      if (!Exec.StreamStep(Target, Step, O.slice, R, &Slots, &Taken)) {
        printf("distill: the executor failed\n");
        return 1;
      }
      Next -= Step.size() - Taken;  // offered again next step
      for (const StreamResult_t &F : R) {
        if (F.tag >= N) return 1;
        Classify(In[F.tag], F.r, X);
        Bufs[F.tag] = {};
        Got++;
      }
    }
  } else {
    const size_t Lanes = std::max<uint32_t>(Exec.Lanes(), 1);
    std::vector<LaneResult> R;
    for (size_t b = 0; b < N; b += Lanes) {
      const size_t n = std::min(Lanes, N - b);
      std::vector<std::vector<uint8_t>> Bufs(n);
      std::vector<std::pair<const uint8_t *, size_t>> Tc(n);
      for (size_t i = 0; i < n; i++) {
        Bufs[i] = ReadFile(In[b + i].path);
        Tc[i] = {Bufs[i].data(), Bufs[i].size()};
      }
      Exec.ResetCoverage();
      if (!Exec.RunBatch(Target, Tc, R, &Slots) || R.size() < n) {
        printf("distill: the executor failed\n");
        return 1;
      }
      for (size_t i = 0; i < n; i++) Classify(In[b + i], &R[i], X);
    }
  }
  const double ReplayMs = MsSince(T0);
  if (Exec.CoverageOverflowed()) {
    printf("distill: a lane's coverage set filled up, so some input's set is incomplete; raise --cov-set (now %u)\n",
           O.cov_set);
    return 1;
  }

  // ---- the cover
  std::vector<uint64_t> Off(N + 1, 0), Values;
  std::vector<uint8_t> Eligible(N, 0);
  uint64_t EligibleN = 0, Entries = 0;
  for (size_t i = 0; i < N; i++) {
    Values.insert(Values.end(), In[i].values.begin(), In[i].values.end());
    Off[i + 1] = Values.size();
    Eligible[i] = In[i].eligible;
    if (In[i].eligible) EligibleN++, Entries += In[i].values.size();
  }
  if (Values.empty()) Values.push_back(0);  // (a pointer to pass; no set reads it)
  const char *HostEnv = getenv("WTFGPU_DISTILL_HOST");
  const bool OnDevice = Exec.HasDeviceDistiller() && !(HostEnv && atoi(HostEnv) == 1);
  std::vector<uint32_t> Index(N), Gain(N);
  uint32_t Kept = 0;
  uint64_t Universe = 0;
  const auto T1 = std::chrono::steady_clock::now();
  const int Rc = OnDevice ? Exec.DeviceDistill((uint32_t)N, Off.data(), Values.data(), Eligible.data(), Index.data(),
                                               Gain.data(), &Kept, &Universe)
                          : wtfdis::distill_host((uint32_t)N, Off.data(), Values.data(), Eligible.data(), Index.data(),
                                                 Gain.data(), &Kept, &Universe);
  const double CoverMs = MsSince(T1);
  if (Rc != 0 || Kept > N) {
    printf("distill: the cover failed (%d)\n", Rc);
    return 1;
  }
  for (uint32_t k = 0; k < Kept; k++) {
    In[Index[k]].order = k;
    In[Index[k]].gain = Gain[k];
  }

  // ---- the output
  fs::create_directories(OutDir, Ec);
  for (uint32_t k = 0; k < Kept; k++) {
    const DistillInput &I = In[Index[k]];
    if (!fs::copy_file(I.path, OutDir / I.name, Ec) || Ec) {
      printf("distill: could not copy %s into %s\n", I.path.string().c_str(), O.output.c_str());
      return 1;
    }
  }
  if (!O.results.empty()) {
    FILE *F = fopen(O.results.c_str(), "w");
    if (!F) {
      printf("distill: could not write %s\n", O.results.c_str());
      return 1;
    }
    for (const DistillInput &I : In)
      fprintf(F, "{\"input\":\"%s\",\"bytes\":%llu,\"result\":\"%s\",\"eligible\":%s,\"values\":%zu,\"kept\":%s,"
                 "\"order\":%lld,\"gain\":%u}\n",
              Escape(I.name).c_str(), (unsigned long long)I.bytes, Escape(I.result).c_str(),
              I.eligible ? "true" : "false", I.values.size(), I.order >= 0 ? "true" : "false", (long long)I.order,
              I.gain);
    fclose(F);
  }
  printf("{\"mode\":\"distill\",\"inputs\":%zu,\"eligible\":%llu,\"kept\":%u,\"universe\":%llu,\"entries\":%llu,"
         "\"rounds\":%llu,\"excluded\":{\"crash\":%llu,\"timeout\":%llu,\"cr3\":%llu,\"error\":%llu,"
         "\"insert_failed\":%llu},\"replay_ms\":%.3f,\"cover_ms\":%.3f,\"on_device\":%s,\"seconds\":%.3f}\n",
         N, (unsigned long long)EligibleN, Kept, (unsigned long long)Universe, (unsigned long long)Entries,
         (unsigned long long)(Universe ? Kept + 1ull : 0ull), (unsigned long long)X.crash,
         (unsigned long long)X.timeout, (unsigned long long)X.cr3, (unsigned long long)X.error,
         (unsigned long long)X.insert_failed, ReplayMs, CoverMs, OnDevice ? "true" : "false", MsSince(T0) / 1000.0);
  return 0;
}

}  // namespace wtfgpu_host
