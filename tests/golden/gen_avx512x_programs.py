#!/usr/bin/env python3
"""Multi-instruction AVX-512 routines, recorded natively (convention U49): the
fixture for the path through k_run — the uop cache, fast loop <-> generic step,
and the cold zmm state both share (tests/test_gpu_avx512x.py).

Four short loops in the style of a vectorised library routine, assembled here
with gcc and run on this host's CPU. Each takes rdi = source, rsi =
destination, rdx = length, rcx = constants, runs a loop whose trip count comes
from the length, has a VEX-encoded xmm move between its EVEX instructions
(the fast loop runs the VEX moves, the generic step the EVEX ones) and ends in
int3:

  rev   byte-reverse copy: vpshufb within the lanes, vpermq across them
  sum   u8 -> u16 widening checksums: vpmovzxbw, vpaddw, vpsrlw / vpsllw
  lut   64-entry u16 table lookup: vpermt2w over two table registers
  tail  masked tail loop: kmovq, vmovdqu8 {k}{z} loads, {k} stores

The native run records, per case, the GPRs at the int3 (from the SIGTRAP
context) and the two destination areas. r11 counts loop trips, so the retired
count the run implies is pre + r11 * loop + post instructions, the three
counts read from the routine's disassembly between its labels.

Output: tests/golden/avx512x_programs.json.gz. Re-run with
    python tests/golden/gen_avx512x_programs.py
"""
import gzip
import json
import os
import random
import re
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "avx512x_programs.json.gz")
SRC_OFF, CONST_OFF, DST_OFF, DST2_OFF, AREA = 0x0000, 0x1000, 0x2000, 0x3000, 0x400
GPRS = ("rax", "rcx", "rdx", "rsi", "rdi", "r8", "r9", "r10", "r11")   # what the routines define
GPR_INDEX = {"rax": 0, "rcx": 1, "rdx": 2, "rsi": 6, "rdi": 7, "r8": 8, "r9": 9, "r10": 10, "r11": 11}

ASM = r"""
.text
.globl r_rev, r_sum, r_lut, r_tail
# ---- byte-reverse copy, 64 bytes a trip (length a multiple of 64)
r_rev:
  mov %rcx, %r10
  xor %eax, %eax
  xor %r11d, %r11d
  vmovdqu64 (%r10), %zmm16            # the in-lane byte reversal
  vmovdqu64 64(%r10), %zmm17          # qwords 6 7 4 5 2 3 0 1: the lanes reversed
r_rev_loop:
  vmovdqu64 (%rdi,%rax), %zmm1
  vpshufb %zmm16, %zmm1, %zmm2
  vmovdqa %xmm2, %xmm3                # VEX
  vpermq %zmm2, %zmm17, %zmm4
  mov %rdx, %r8
  sub %rax, %r8
  vmovdqu64 %zmm4, -64(%rsi,%r8)
  vmovdqu %xmm3, 0x1000(%rsi,%rax)    # VEX
  inc %r11
  add $64, %rax
  cmp %rdx, %rax
  jb r_rev_loop
r_rev_post:
  vmovq %xmm3, %r9                    # VEX
  int3
# ---- u8 -> u16 widening checksums, 32 bytes a trip (length a multiple of 32)
r_sum:
  mov %rcx, %r10
  xor %eax, %eax
  xor %r11d, %r11d
  vpxord %zmm0, %zmm0, %zmm0
  vpxord %zmm18, %zmm18, %zmm18
r_sum_loop:
  vpmovzxbw (%rdi,%rax), %zmm1
  vpaddw %zmm1, %zmm0, %zmm0
  vmovdqa %xmm0, %xmm5                # VEX
  vpsrlw $1, %zmm1, %zmm2
  vpsllw $3, %zmm1, %zmm3
  vpxord %zmm2, %zmm3, %zmm3
  vpaddw %zmm3, %zmm18, %zmm18
  inc %r11
  add $32, %rax
  cmp %rdx, %rax
  jb r_sum_loop
r_sum_post:
  vmovdqu64 %zmm0, (%rsi)
  vmovdqu64 %zmm18, 64(%rsi)
  vmovd %xmm5, %r8d                   # VEX
  vpsrlq $32, %zmm18, %zmm19
  vmovq %xmm19, %r9                   # EVEX
  int3
# ---- 64-entry u16 table lookup, 32 indices a trip (length in elements, a multiple of 32)
r_lut:
  mov %rcx, %r10
  xor %r8d, %r8d
  xor %eax, %eax
  xor %r11d, %r11d
  vmovdqu64 128(%r10), %zmm20
  vmovdqu64 192(%r10), %zmm21
r_lut_loop:
  vmovdqu16 (%rdi,%rax,2), %zmm1
  vmovdqa64 %zmm20, %zmm2
  vpermt2w %zmm21, %zmm1, %zmm2
  vmovdqa %xmm2, %xmm3                # VEX
  vmovdqu16 %zmm2, (%rsi,%rax,2)
  vmovdqu %xmm3, 0x1000(%rsi,%rax,2)  # VEX
  inc %r11
  add $32, %rax
  cmp %rdx, %rax
  jb r_lut_loop
r_lut_post:
  vmovq %xmm3, %r9                    # VEX
  int3
# ---- masked tail loop, up to 64 bytes a trip (any length)
r_tail:
  mov %rcx, %r10
  xor %eax, %eax
  xor %r11d, %r11d
  vpbroadcastb 256(%r10), %zmm22
r_tail_loop:
  mov %rdx, %rcx
  sub %rax, %rcx
  mov $64, %r9d
  cmp %r9, %rcx
  cmova %r9, %rcx
  mov $-1, %r8
  mov $1, %r9d
  shl %cl, %r9
  dec %r9
  cmp $64, %rcx
  cmovb %r9, %r8
  kmovq %r8, %k1
  vmovdqu8 (%rdi,%rax), %zmm1{%k1}{z}
  vmovdqa %xmm1, %xmm3                # VEX
  vpaddb %zmm22, %zmm1, %zmm1{%k1}
  vmovdqu8 %zmm1, (%rsi,%rax){%k1}
  inc %r11
  add $64, %rax
  cmp %rdx, %rax
  jb r_tail_loop
r_tail_post:
  kmovq %k1, %r8
  vmovq %xmm3, %r9                    # VEX
  int3
r_end:
"""

HARNESS = r"""
#define _GNU_SOURCE
#include <setjmp.h>
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <ucontext.h>
void r_rev(void), r_sum(void), r_lut(void), r_tail(void);
typedef void (*fn_t)(void *, void *, uint64_t, void *);
static fn_t fns[] = {(fn_t)r_rev, (fn_t)r_sum, (fn_t)r_lut, (fn_t)r_tail};
static uint8_t g_buf[0x4000] __attribute__((aligned(4096)));
static sigjmp_buf g_jb;
static volatile uint64_t g_r[9];
static void on_trap(int sig, siginfo_t *si, void *uc) {
  greg_t *g = ((ucontext_t *)uc)->uc_mcontext.gregs;
  const int idx[9] = {REG_RAX, REG_RCX, REG_RDX, REG_RSI, REG_RDI, REG_R8, REG_R9, REG_R10, REG_R11};
  for (int i = 0; i < 9; i++) g_r[i] = (uint64_t)g[idx[i]];
  siglongjmp(g_jb, 1);
}
int main(void) {
  struct sigaction sa;
  memset(&sa, 0, sizeof(sa));
  sa.sa_sigaction = on_trap;
  sa.sa_flags = SA_SIGINFO | SA_NODEFER;
  sigaction(SIGTRAP, &sa, 0);
  printf("BUF %llx\n", (unsigned long long)(uintptr_t)g_buf);
  int r;
  unsigned long long len;
  unsigned int b;
  while (scanf("%d %llu", &r, &len) == 2) {
    memset(g_buf, 0, sizeof(g_buf));
    for (int i = 0; i < 0x800; i++) { if (scanf("%2x", &b) != 1) return 1; g_buf[i] = (uint8_t)b; }
    for (int i = 0; i < 0x200; i++) { if (scanf("%2x", &b) != 1) return 1; g_buf[0x1000 + i] = (uint8_t)b; }
    if (!sigsetjmp(g_jb, 1)) fns[r](g_buf, g_buf + 0x2000, len, g_buf + 0x1000);
    __asm__ volatile("vzeroupper");
    printf("G");
    for (int i = 0; i < 9; i++) printf(" %llx", (unsigned long long)g_r[i]);
    printf("\nD");
    for (int i = 0; i < 0x400; i++) printf("%02x", g_buf[0x2000 + i]);
    printf("\nE");
    for (int i = 0; i < 0x400; i++) printf("%02x", g_buf[0x3000 + i]);
    printf("\n");
  }
  return 0;
}
"""

ROUTINES = ("rev", "sum", "lut", "tail")
LENGTHS = {"rev": (64, 128, 192, 256, 320, 384, 448, 512), "sum": (32, 96, 160, 224, 288, 352, 416, 480),
           "lut": (32, 64, 96, 128, 160, 192, 224, 256), "tail": (1, 17, 63, 64, 65, 130, 255, 300)}


def constants():
    """0: the in-lane byte reversal; 64: the lane-reversing qword indices (high
    bits set: vpermq takes the low three); 128: the 64-entry u16 table; 256:
    the byte the tail loop adds."""
    rng = random.Random(0x512C)
    c = bytearray(0x200)
    c[0:64] = bytes(15 - (i & 15) for i in range(64))
    for i, q in enumerate((6, 7, 4, 5, 2, 3, 0, 1)):
        c[64 + 8 * i: 72 + 8 * i] = (q | 0xA5A5A5A5A5A5A5A8).to_bytes(8, "little")
    c[128:256] = rng.randbytes(128)
    c[256] = 0x5B
    return bytes(c)


def source(routine, seed):
    """The 0x800-byte source area of a case."""
    return random.Random(seed).randbytes(0x800)


def model(routine, n, src, consts):
    """What the routine leaves in its first destination area (a check on the routine itself)."""
    out = bytearray(AREA)
    if routine == "rev":
        out[:n] = src[:n][::-1]
    elif routine == "sum":
        acc, acc2 = [0] * 32, [0] * 32
        for t in range(n // 32):
            for j in range(32):
                v = src[32 * t + j]
                acc[j] = (acc[j] + v) & 0xFFFF
                acc2[j] = (acc2[j] + ((v >> 1) ^ ((v << 3) & 0xFFFF))) & 0xFFFF
        out[:128] = b"".join(v.to_bytes(2, "little") for v in acc + acc2)
    elif routine == "lut":
        tab = [int.from_bytes(consts[128 + 2 * i: 130 + 2 * i], "little") for i in range(64)]
        for i in range(n):
            idx = int.from_bytes(src[2 * i: 2 * i + 2], "little") & 63
            out[2 * i: 2 * i + 2] = tab[idx].to_bytes(2, "little")
    else:
        out[:n] = bytes((v + consts[256]) & 0xFF for v in src[:n])
    return bytes(out)


def assemble(td):
    s, o = os.path.join(td, "r.S"), os.path.join(td, "r.o")
    with open(s, "w") as f:
        f.write(ASM)
    subprocess.check_call(["gcc", "-c", "-o", o, s])
    binp = os.path.join(td, "r.bin")
    subprocess.check_call(["objcopy", "-O", "binary", "-j", ".text", o, binp])
    code = open(binp, "rb").read()
    sym = {}
    for line in subprocess.check_output(["nm", o], text=True).split("\n"):
        p = line.split()
        if len(p) == 3:
            sym[p[2]] = int(p[0], 16)
    insns = []   # (address, mnemonic)
    for line in subprocess.check_output(["objdump", "-d", "--insn-width=16", o], text=True).split("\n"):
        m = re.match(r"\s*([0-9a-f]+):\t[0-9a-f ]+\t(\S+)", line)
        if m:
            insns.append((int(m.group(1), 16), m.group(2)))
    return o, code[:sym["r_end"]], sym, insns


def main():
    consts = constants()
    with tempfile.TemporaryDirectory() as td:
        obj, code, sym, insns = assemble(td)
        exe = os.path.join(td, "h")
        with open(os.path.join(td, "h.c"), "w") as f:
            f.write(HARNESS)
        subprocess.check_call(["gcc", "-O1", "-no-pie", "-o", exe, os.path.join(td, "h.c"), obj])
        cases = [(r, n, 0xC0DE00 + 16 * ri + j) for ri, r in enumerate(ROUTINES) for j, n in enumerate(LENGTHS[r])]
        lines = ["%d %d %s %s" % (ROUTINES.index(r), n, source(r, seed).hex(), consts.hex()) for r, n, seed in cases]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                             check=True).stdout.split("\n")
    buf_va = int(out[0].split()[1], 16)

    def count(a, b):
        return sum(1 for addr, _ in insns if a <= addr < b)

    routines = {}
    for r in ROUTINES:
        a, lp, po = sym["r_" + r], sym[f"r_{r}_loop"], sym[f"r_{r}_post"]
        end = min(addr for addr, mn in insns if addr >= po and mn == "int3")
        routines[r] = {"entry": a, "pre": count(a, lp), "loop": count(lp, po), "post": count(po, end)}
    doc = {"buf_va": "%x" % buf_va, "code": code.hex(), "consts": consts.hex(), "routines": routines,
           "layout": {"src": SRC_OFF, "consts": CONST_OFF, "dst": DST_OFF, "dst2": DST2_OFF, "area": AREA},
           "gprs": list(GPRS), "generator": "tests/golden/gen_avx512x_programs.py", "cases": []}
    for k, (r, n, seed) in enumerate(cases):
        g = [int(v, 16) for v in out[1 + 3 * k].split()[1:]]
        dst, dst2 = bytes.fromhex(out[2 + 3 * k][1:]), bytes.fromhex(out[3 + 3 * k][1:])
        assert dst == model(r, n, source(r, seed), consts), (r, n)
        trips = g[GPRS.index("r11")]
        rt = routines[r]
        doc["cases"].append({"routine": r, "len": n, "seed": seed,
                             "gpr": ["%x" % v for v in g], "dst": dst.hex(), "dst2": dst2.hex(),
                             "icount": rt["pre"] + trips * rt["loop"] + rt["post"]})
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(f"wrote {len(cases)} program cases, {len(code)} code bytes, to {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
