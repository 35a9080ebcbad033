// keep_filter_main.cc — TEST INFRASTRUCTURE ONLY: KeepsTestcase
// (wtf_amd/host/runner.h), the one decision behind FuzzSession::AccountStep's
// serial results and the device executor's read-back filter, over the kinds
// of result a campaign sees. Header-only: nothing of the host library is
// linked. Prints "<case> <0|1>" per case, then "ok".
#include <cstdio>

#include "../../wtf_amd/host/runner.h"

using namespace wtfgpu_host;

int main() {
  const std::unordered_set<std::string> known{"crash-known"};
  const auto make = [](TestcaseResult_t R, bool error, bool cov) {
    LaneResult L;
    L.result = std::move(R);
    L.error = error;
    if (cov) L.new_coverage = {0x1000, 0x1004};
    return L;
  };
  struct Case {
    const char *name;
    LaneResult L;
  };
  const Case cases[] = {
      {"error", make(Crash_t(), true, false)},
      {"error_with_coverage", make(Ok_t(), true, true)},
      {"timeout", make(Timedout_t(), false, false)},
      {"timeout_with_coverage", make(Timedout_t(), false, true)},
      {"crash_known_name", make(Crash_t("crash-known"), false, false)},
      {"crash_known_name_with_coverage", make(Crash_t("crash-known"), false, true)},
      {"crash_new_name", make(Crash_t("crash-new"), false, false)},
      {"crash_empty_name", make(Crash_t(), false, false)},
      {"ok", make(Ok_t(), false, false)},
      {"ok_with_coverage", make(Ok_t(), false, true)},
      {"cr3", make(Cr3Change_t(), false, false)},
      {"cr3_with_coverage", make(Cr3Change_t(), false, true)},
  };
  for (const Case &c : cases) printf("%s %d\n", c.name, KeepsTestcase(&c.L, false, known) ? 1 : 0);
  for (const Case &c : cases) printf("every_%s %d\n", c.name, KeepsTestcase(&c.L, true, known) ? 1 : 0);
  printf("plain %d\n", KeepsTestcase(nullptr, false, known) ? 1 : 0);
  printf("every_plain %d\n", KeepsTestcase(nullptr, true, known) ? 1 : 0);
  // the set is read at the call: a name is new until it is inserted
  std::unordered_set<std::string> grows;
  const LaneResult L = make(Crash_t("crash-new"), false, false);
  printf("before_insert %d\n", KeepsTestcase(&L, false, grows) ? 1 : 0);
  grows.insert("crash-new");
  printf("after_insert %d\n", KeepsTestcase(&L, false, grows) ? 1 : 0);
  puts("ok");
  return 0;
}
