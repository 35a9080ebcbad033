#!/usr/bin/env python3
"""Records tests/golden/stream_campaigns.json: fixed-seed streaming campaigns
of the GPU node (`wtfgpu fuzz --seed 1337 --runs N`) that every later build
must reproduce exactly (tests/test_gpu_stream_pinned.py). Run it on an MI355X
from the commit whose results are the reference:

    python scripts/gen_stream_campaigns.py [OUT.json]

Per config it stores the summary counts, the kernel's group_steps and the
sorted file names under crashes/ and outputs/. Each config is run twice. A
key on which the recording build disagrees with itself is not a property
later builds can be held to: it is listed under "unstable" and kept out of
"expect" (a tlv config must reproduce every key, or the recording fails)."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import tlv_harness as H  # noqa: E402

KEYS = ("execs", "retired", "coverage", "corpus", "crashes", "unique_crashes", "timeouts", "cr3", "errors",
        "error_retired")

# 256 lanes is the smallest count that pipelines (two halves of two waves);
# with 256-step slices lanes live across several slices, so every harvest sees
# a partly finished part. 16,384 lanes: halves of 8,192 cross every "parallel
# above N lanes" threshold of the host loops.
_SHORT = ["--slice-steps", "256", "--regroup-steps", "64"]
CONFIGS = [
    {"id": "tlv_256_short_slices", "target": "tlv", "name": "tlv_server", "lanes": 256, "runs": 8192,
     "limit": 100000, "max_len": 0x1000, "extra": _SHORT, "env": {}},
    {"id": "tlv_256_short_slices_host_bp", "target": "tlv", "name": "tlv_server", "lanes": 256, "runs": 8192,
     "limit": 100000, "max_len": 0x1000, "extra": _SHORT, "env": {"WTFGPU_DEVICE_BP_ACTIONS": "0"}},
    {"id": "tlv_16384", "target": "tlv", "name": "tlv_server", "lanes": 16384, "runs": 49152,
     "limit": 100000, "max_len": 0x1000, "extra": [], "env": {}},
    {"id": "hevd_bare_256", "target": "hevd", "name": "hevd", "lanes": 256, "runs": 32768,
     "limit": 10000000, "max_len": 1028, "extra": [], "env": {}},
    {"id": "hevd_bare_16384", "target": "hevd", "name": "hevd", "lanes": 16384, "runs": 32768,
     "limit": 10000000, "max_len": 1028, "extra": [], "env": {}},
    # the one-part path (no pipelining: the harvest runs in the refill's call
    # and reads the exits, counts and StopWithArgs arguments itself)
    {"id": "tlv_256_short_slices_one_part", "target": "tlv", "name": "tlv_server", "lanes": 256, "runs": 8192,
     "limit": 100000, "max_len": 0x1000, "extra": _SHORT, "env": {"WTFGPU_STREAM_PARTS": "1"}},
    {"id": "hevd_bare_256_one_part", "target": "hevd", "name": "hevd", "lanes": 256, "runs": 32768,
     "limit": 10000000, "max_len": 1028, "extra": [], "env": {"WTFGPU_STREAM_PARTS": "1"}},
]

_BUILD = {"tlv": H.build_target, "hevd": H.build_hevd_target}


def build_bases(tmp, kinds):
    """One snapshot directory per target kind, shared by that kind's configs."""
    return {k: _BUILD[k](os.path.join(tmp, "base_" + k)) for k in sorted(set(kinds))}


def run_config(cfg, base, work):
    """One campaign of cfg on a fresh copy of the snapshot `base`: the record the fixture keeps."""
    shutil.copytree(base, work, ignore=shutil.ignore_patterns("outputs", "crashes", "errors"))
    cmd = [H.WTFGPU, "fuzz", "--name", cfg["name"], "--target", work, "--runs", str(cfg["runs"]),
           "--lanes", str(cfg["lanes"]), "--seed", "1337", "--limit", str(cfg["limit"]),
           "--max_len", str(cfg["max_len"]), *cfg["extra"]]
    out = subprocess.run(cmd, check=True, timeout=300, capture_output=True, text=True,
                         env={**os.environ, **cfg["env"]}).stdout
    st = json.loads([line for line in out.splitlines() if line.startswith("{")][-1])

    def names(sub):
        p = os.path.join(work, sub)
        return sorted(os.listdir(p)) if os.path.isdir(p) else []

    rec = {k: st[k] for k in KEYS}
    rec["group_steps"] = st["backend"]["group_steps"]
    rec["crash_names"] = names("crashes")
    rec["output_names"] = names("outputs")
    return rec


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "stream_campaigns.json")
    fixture = {"configs": []}
    with tempfile.TemporaryDirectory() as tmp:
        bases = build_bases(tmp, [c["target"] for c in CONFIGS])
        for cfg in CONFIGS:
            a = run_config(cfg, bases[cfg["target"]], os.path.join(tmp, cfg["id"] + "_a"))
            b = run_config(cfg, bases[cfg["target"]], os.path.join(tmp, cfg["id"] + "_b"))
            unstable = sorted(k for k in a if a[k] != b[k])
            if unstable and cfg["target"] == "tlv":
                sys.exit(f"{cfg['id']}: NOT reproducible (differs in {unstable})")
            if unstable:
                print(f"{cfg['id']}: differs from itself in {unstable}: {[(a[k], b[k]) for k in unstable]}",
                      flush=True)
            print(f"{cfg['id']}: execs {a['execs']} crashes {a['crashes']} corpus {a['corpus']} "
                  f"errors {a['errors']} group_steps {a['group_steps']}", flush=True)
            fixture["configs"].append({"config": cfg, "unstable": unstable,
                                       "expect": {k: v for k, v in a.items() if k not in unstable}})
    with open(out, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {len(fixture['configs'])} of {len(CONFIGS)} configs")


if __name__ == "__main__":
    main()
