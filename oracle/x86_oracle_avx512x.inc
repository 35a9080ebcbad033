/*
 * x86_oracle_avx512x.inc — the AVX-512 integer forms of convention U49 in the
 * oracle (DESIGN.md §5; the engine's wtf_amd/csrc/engine_avx512x.h). Included
 * by x86_oracle.c after x86_oracle_avx512.inc, whose helpers it uses; TEST
 * INFRASTRUCTURE ONLY like the rest of the oracle. Pinned by native execution
 * on an AVX-512 host (tests/golden/gen_avx512x_vectors.py and
 * gen_avx512x_programs.py, through tests/test_avx512x.py).
 *
 * Restated from the SDM's operation sections, one instruction page at a time,
 * as whole-vector scalar C: every form first computes its unmasked result
 * from whole source vectors (xcompute), and one place applies the opmask
 * (exec_evexx). Families:
 *   A  vpmin / vpmax (s u; b w d q), vpabs, vpadds / vpaddus / vpsubs /
 *      vpsubus, vpavg, vpmullw / vpmulhw / vpmulhuw / vpmulld / vpmullq,
 *      vpmuludq / vpmuldq
 *   B  vpsrl / vpsra / vpsll by imm8, by the low qword of an xmm / m128 and
 *      per element (vpsrlv ...), vprol / vpror (imm8, per element), vpslldq /
 *      vpsrldq
 *   C  vpshufb / d / hw / lw, vpunpck l / h, vpackss / vpackus, vpalignr —
 *      each within its 128-bit lane
 *   D  vpermb / w / d / q, vpermq imm8, vpermi2 / vpermt2, valignd / q,
 *      vshufi32x4 / 64x2
 *   E  vpmovzx / vpmovsx
 *   F  vinserti / vextracti / vbroadcasti 32x4 64x2 32x8 64x4, vbroadcasti32x2
 *   G  vpmovm2b / w / d / q, vpmovb / w / d / q2m
 *   H  vmovd / vmovq
 *
 * The common rules (SDM vol. 2 §2.7, §2.8; x86_oracle_avx512.inc's header):
 *   - #UD: L'L = 11 or a length the form does not have, EVEX.W where the form
 *     fixes it, an undefined /digit of the 71 / 72 / 73 groups, vvvv != 11111
 *     (V' included) on a two-operand form, EVEX.b without a broadcastable
 *     memory operand, z without a mask or with a memory destination, a mask
 *     on a form that takes none (vpslldq / vpsrldq, G, H), a register where
 *     only memory is defined (vbroadcasti 32x4 ...) and the reverse (G); then
 *     #NM, then the memory operand.
 *   - memory fault suppression applies where a destination element depends on
 *     one source element only (A, B's element shifts, E, vbroadcasti); the
 *     forms that move elements about (C, D, the xmm count) read their whole
 *     operand whatever the mask, and so do vinserti's block load and
 *     vextracti's block store (class E6NF: the store checks the whole block
 *     and writes the selected elements).
 *   - disp8 * N: the broadcast element with EVEX.b, else the memory operand's
 *     whole size (the vector, a half / quarter / eighth for E, 16 for the xmm
 *     count and the 128-bit blocks, 32 for the 256-bit ones, 8 / 4 for
 *     vbroadcasti32x2 and H).
 */

enum {
  XK_NONE, XK_BADDIGIT,
  /* A */ XK_MINS, XK_MAXS, XK_MINU, XK_MAXU, XK_ABS, XK_ADDS, XK_ADDUS, XK_SUBS, XK_SUBUS, XK_AVG, XK_MULLO, XK_MULHS,
  XK_MULHU, XK_MULUDQ, XK_MULDQ,
  /* B */ XK_SRL, XK_SRA, XK_SLL, XK_ROL, XK_ROR, XK_BSRL, XK_BSLL,
  /* C */ XK_SHUFB, XK_SHUFD, XK_SHUFHW, XK_SHUFLW, XK_UNPCKL, XK_UNPCKH, XK_PACKSS, XK_PACKUS, XK_ALIGNR,
  /* D */ XK_PERM, XK_PERMQI, XK_PERMI2, XK_PERMT2, XK_VALIGN, XK_SHUFI,
  /* E */ XK_MOVZX, XK_MOVSX,
  /* F */ XK_INSERT, XK_EXTRACT, XK_BCBLK,
  /* G */ XK_M2V, XK_V2M,
  /* H */ XK_GPR2X, XK_X2GPR, XK_MOVQ_LD, XK_MOVQ_ST
};
enum { XC_ELEM, XC_IMM, XC_XMM }; /* where a shift's count comes from */

typedef struct {
  int kind;
  u32 es;      /* the element the opmask counts (bytes) */
  u32 ses;     /* source element bytes where they differ (packs, E), else es */
  u32 bc;      /* embedded broadcast element bytes, 0 = EVEX.b is #UD */
  int wreq;    /* EVEX.W the form requires, -1 = ignored */
  int shape;   /* 3: reg, vvvv, r/m; 2: reg, r/m; 1: vvvv, r/m with a /digit */
  int cnt;     /* XC_* for the shifts */
  u32 minll, maxll;
  int nomask, memonly, regonly;
  u32 mfix;    /* memory operand bytes at every length, 0 = the vector's (divided by es / ses for E) */
  int whole;   /* the memory operand is read whole, whatever the mask */
  int has_imm;
} xform;

static xform xf_mk(int kind, u32 es, u32 bc, int wreq, int shape) {
  xform f;
  memset(&f, 0, sizeof f);
  f.kind = kind;
  f.es = f.ses = es;
  f.bc = bc;
  f.wreq = wreq;
  f.shape = shape;
  f.maxll = 2;
  return f;
}

/* digit: ModRM.reg[2:0] for the 71 / 72 / 73 groups, -1 before ModRM is read
 * (any defined digit's form stands in: only has_imm is asked then). */
static xform xform_of(u32 map, u32 op, int pp, u32 w, int digit) {
  const xform none = xf_mk(XK_NONE, 0, 0, -1, 3);
  const u32 dq = w ? 8 : 4;
  xform f = none;
#define XF(k, e, b, wr, sh) (f = xf_mk((k), (e), (b), (wr), (sh)))
  if (map == 1 && pp == 1) {
    switch (op) {
    /* A */
    case 0xea: XF(XK_MINS, 2, 0, -1, 3); break;
    case 0xee: XF(XK_MAXS, 2, 0, -1, 3); break;
    case 0xd8: XF(XK_SUBUS, 1, 0, -1, 3); break;
    case 0xd9: XF(XK_SUBUS, 2, 0, -1, 3); break;
    case 0xdc: XF(XK_ADDUS, 1, 0, -1, 3); break;
    case 0xdd: XF(XK_ADDUS, 2, 0, -1, 3); break;
    case 0xe8: XF(XK_SUBS, 1, 0, -1, 3); break;
    case 0xe9: XF(XK_SUBS, 2, 0, -1, 3); break;
    case 0xec: XF(XK_ADDS, 1, 0, -1, 3); break;
    case 0xed: XF(XK_ADDS, 2, 0, -1, 3); break;
    case 0xe0: XF(XK_AVG, 1, 0, -1, 3); break;
    case 0xe3: XF(XK_AVG, 2, 0, -1, 3); break;
    case 0xd5: XF(XK_MULLO, 2, 0, -1, 3); break;
    case 0xe5: XF(XK_MULHS, 2, 0, -1, 3); break;
    case 0xe4: XF(XK_MULHU, 2, 0, -1, 3); break;
    case 0xf4: XF(XK_MULUDQ, 8, 8, 1, 3); break;
    /* B: the count in an xmm / m128 */
    case 0xd1: case 0xd2: case 0xd3: case 0xe1: case 0xe2: case 0xf1: case 0xf2: case 0xf3: {
      const u32 lo = op & 15;
      const int k = (op >> 4) == 0xd ? XK_SRL : (op >> 4) == 0xe ? XK_SRA : XK_SLL;
      if (lo == 1) XF(k, 2, 0, -1, 3);
      else if (k == XK_SRA) XF(k, dq, 0, -1, 3); /* e2: vpsrad (W0) / vpsraq (W1) */
      else XF(k, lo == 2 ? 4 : 8, 0, lo == 2 ? 0 : 1, 3);
      f.cnt = XC_XMM;
      f.mfix = 16;
      f.whole = 1;
      break;
    }
    /* B: the imm8 groups */
    case 0x71:
      if (digit < 0) digit = 2;
      if (digit == 2 || digit == 4 || digit == 6) XF(digit == 2 ? XK_SRL : digit == 4 ? XK_SRA : XK_SLL, 2, 0, -1, 1);
      else XF(XK_BADDIGIT, 2, 0, -1, 1);
      f.cnt = XC_IMM;
      f.has_imm = 1;
      break;
    case 0x72:
      if (digit < 0) digit = 2;
      if (digit == 0 || digit == 1) XF(digit ? XK_ROL : XK_ROR, dq, dq, -1, 1);
      else if (digit == 4) XF(XK_SRA, dq, dq, -1, 1);
      else if (digit == 2 || digit == 6) XF(digit == 2 ? XK_SRL : XK_SLL, 4, 4, 0, 1);
      else XF(XK_BADDIGIT, 4, 0, -1, 1);
      f.cnt = XC_IMM;
      f.has_imm = 1;
      break;
    case 0x73:
      if (digit < 0) digit = 2;
      if (digit == 2 || digit == 6) XF(digit == 2 ? XK_SRL : XK_SLL, 8, 8, 1, 1);
      else if (digit == 3 || digit == 7) {
        XF(digit == 3 ? XK_BSRL : XK_BSLL, 1, 0, -1, 1);
        f.nomask = 1;
        f.whole = 1;
      } else XF(XK_BADDIGIT, 8, 0, -1, 1);
      f.cnt = XC_IMM;
      f.has_imm = 1;
      break;
    /* C */
    case 0x70: XF(XK_SHUFD, 4, 4, 0, 2); f.has_imm = 1; f.whole = 1; break;
    case 0x60: case 0x61: case 0x68: case 0x69:
      XF(op < 0x68 ? XK_UNPCKL : XK_UNPCKH, 1u << (op & 1), 0, -1, 3);
      f.whole = 1;
      break;
    case 0x62: case 0x6a: XF(op == 0x62 ? XK_UNPCKL : XK_UNPCKH, 4, 4, 0, 3); f.whole = 1; break;
    case 0x6c: case 0x6d: XF(op == 0x6c ? XK_UNPCKL : XK_UNPCKH, 8, 8, 1, 3); f.whole = 1; break;
    case 0x63: XF(XK_PACKSS, 1, 0, -1, 3); f.ses = 2; f.whole = 1; break;
    case 0x67: XF(XK_PACKUS, 1, 0, -1, 3); f.ses = 2; f.whole = 1; break;
    case 0x6b: XF(XK_PACKSS, 2, 4, 0, 3); f.ses = 4; f.whole = 1; break;
    /* H */
    case 0x6e: XF(XK_GPR2X, dq, 0, -1, 2); f.mfix = dq; f.maxll = 0; f.nomask = 1; break;
    case 0x7e: XF(XK_X2GPR, dq, 0, -1, 2); f.mfix = dq; f.maxll = 0; f.nomask = 1; break;
    case 0xd6: XF(XK_MOVQ_ST, 8, 0, 1, 2); f.mfix = 8; f.maxll = 0; f.nomask = 1; break;
    default: break;
    }
  } else if (map == 1 && pp == 2) {
    if (op == 0x70) { XF(XK_SHUFHW, 2, 0, -1, 2); f.has_imm = 1; f.whole = 1; }
    else if (op == 0x7e) { XF(XK_MOVQ_LD, 8, 0, 1, 2); f.mfix = 8; f.maxll = 0; f.nomask = 1; }
  } else if (map == 1 && pp == 3) {
    if (op == 0x70) { XF(XK_SHUFLW, 2, 0, -1, 2); f.has_imm = 1; f.whole = 1; }
  } else if (map == 2 && pp == 1) {
    switch (op) {
    case 0x00: XF(XK_SHUFB, 1, 0, -1, 3); f.whole = 1; break;
    case 0x10: XF(XK_SRL, 2, 0, 1, 3); break;
    case 0x11: XF(XK_SRA, 2, 0, 1, 3); break;
    case 0x12: XF(XK_SLL, 2, 0, 1, 3); break;
    case 0x14: XF(XK_ROR, dq, dq, -1, 3); break;
    case 0x15: XF(XK_ROL, dq, dq, -1, 3); break;
    case 0x45: XF(XK_SRL, dq, dq, -1, 3); break;
    case 0x46: XF(XK_SRA, dq, dq, -1, 3); break;
    case 0x47: XF(XK_SLL, dq, dq, -1, 3); break;
    case 0x1c: XF(XK_ABS, 1, 0, -1, 2); break;
    case 0x1d: XF(XK_ABS, 2, 0, -1, 2); break;
    case 0x1e: XF(XK_ABS, 4, 4, 0, 2); break;
    case 0x1f: XF(XK_ABS, 8, 8, 1, 2); break;
    case 0x20: case 0x21: case 0x22: case 0x23: case 0x24: case 0x25:
    case 0x30: case 0x31: case 0x32: case 0x33: case 0x34: case 0x35: {
      static const u8 des[6] = {2, 4, 8, 4, 8, 8}, ses[6] = {1, 1, 1, 2, 2, 4};
      const u32 t = op & 7;
      XF(op < 0x30 ? XK_MOVSX : XK_MOVZX, des[t], 0, t == 5 ? 0 : -1, 2);
      f.ses = ses[t];
      break;
    }
    case 0x28: XF(XK_MULDQ, 8, 8, 1, 3); break;
    case 0x2b: XF(XK_PACKUS, 2, 4, 0, 3); f.ses = 4; f.whole = 1; break;
    case 0x36: XF(XK_PERM, dq, dq, -1, 3); f.minll = 1; f.whole = 1; break;
    case 0x8d: XF(XK_PERM, w ? 2 : 1, 0, -1, 3); f.whole = 1; break;
    case 0x75: XF(XK_PERMI2, w ? 2 : 1, 0, -1, 3); f.whole = 1; break;
    case 0x76: XF(XK_PERMI2, dq, dq, -1, 3); f.whole = 1; break;
    case 0x7d: XF(XK_PERMT2, w ? 2 : 1, 0, -1, 3); f.whole = 1; break;
    case 0x7e: XF(XK_PERMT2, dq, dq, -1, 3); f.whole = 1; break;
    case 0x38: XF(XK_MINS, 1, 0, -1, 3); break;
    case 0x3c: XF(XK_MAXS, 1, 0, -1, 3); break;
    case 0x39: XF(XK_MINS, dq, dq, -1, 3); break;
    case 0x3d: XF(XK_MAXS, dq, dq, -1, 3); break;
    case 0x3b: XF(XK_MINU, dq, dq, -1, 3); break;
    case 0x3f: XF(XK_MAXU, dq, dq, -1, 3); break;
    case 0x40: XF(XK_MULLO, dq, dq, -1, 3); break;
    case 0x59: if (!w) { XF(XK_BCBLK, 4, 0, 0, 2); f.mfix = 8; } break; /* vbroadcasti32x2 (W1: vpbroadcastq, U47) */
    case 0x5a: XF(XK_BCBLK, dq, 0, -1, 2); f.mfix = 16; f.minll = 1; f.memonly = 1; break;
    case 0x5b: XF(XK_BCBLK, dq, 0, -1, 2); f.mfix = 32; f.minll = 2; f.memonly = 1; break;
    default: break;
    }
  } else if (map == 2 && pp == 2) {
    if (op == 0x28 || op == 0x38) { XF(XK_M2V, op == 0x28 ? (w ? 2 : 1) : dq, 0, -1, 2); f.nomask = f.regonly = 1; }
    else if (op == 0x29 || op == 0x39) { XF(XK_V2M, op == 0x29 ? (w ? 2 : 1) : dq, 0, -1, 2); f.nomask = f.regonly = 1; }
  } else if (map == 3 && pp == 1) {
    switch (op) {
    case 0x00: XF(XK_PERMQI, 8, 8, 1, 2); f.minll = 1; f.whole = 1; break;
    case 0x03: XF(XK_VALIGN, dq, dq, -1, 3); f.whole = 1; break;
    case 0x0f: XF(XK_ALIGNR, 1, 0, -1, 3); f.whole = 1; break;
    case 0x43: XF(XK_SHUFI, dq, dq, -1, 3); f.minll = 1; f.whole = 1; break;
    case 0x38: XF(XK_INSERT, dq, 0, -1, 3); f.mfix = 16; f.minll = 1; f.whole = 1; break;
    case 0x3a: XF(XK_INSERT, dq, 0, -1, 3); f.mfix = 32; f.minll = 2; f.whole = 1; break;
    case 0x39: XF(XK_EXTRACT, dq, 0, -1, 2); f.mfix = 16; f.minll = 1; break;
    case 0x3b: XF(XK_EXTRACT, dq, 0, -1, 2); f.mfix = 32; f.minll = 2; break;
    default: break;
    }
    if (f.kind != XK_NONE) f.has_imm = 1;
  }
#undef XF
  return f;
}

/* The memory operand's bytes at vector length vlb. */
static u32 xf_msize(const xform *f, u32 vlb) {
  if (f->mfix) return f->mfix;
  if (f->kind == XK_MOVZX || f->kind == XK_MOVSX) return vlb / (f->es / f->ses);
  return vlb;
}
static u32 xdisp_n(const xform *f, u32 vlb, u32 b) { return (b && f->bc) ? f->bc : xf_msize(f, vlb); }

static u64 xmask_bits(u32 bits) { return bits >= 64 ? ~0ULL : (1ULL << bits) - 1; }
static i64 xsat_s(i64 v, u32 bits) {
  const i64 hi = (i64)(xmask_bits(bits - 1)), lo = -hi - 1;
  return v > hi ? hi : v < lo ? lo : v;
}
static u64 xsat_u(i64 v, u32 bits) { return v < 0 ? 0 : (u64)v > xmask_bits(bits) ? xmask_bits(bits) : (u64)v; }

/* One element of a logical / arithmetic shift or a rotate: the count as the
 * instruction page gives it (a count above width - 1 shifts everything out,
 * or fills with the sign; a rotate takes it modulo the width). */
static u64 xshift(int kind, u64 x, u64 cnt, u32 bits) {
  const u64 mk = xmask_bits(bits);
  x &= mk;
  switch (kind) {
  case XK_SRL: return cnt >= bits ? 0 : x >> cnt;
  case XK_SLL: return cnt >= bits ? 0 : (x << cnt) & mk;
  case XK_SRA: {
    const int neg = (int)((x >> (bits - 1)) & 1);
    if (cnt >= bits) return neg ? mk : 0;
    return ((x >> cnt) | (neg && cnt ? mk << (bits - cnt) : 0)) & mk;
  }
  case XK_ROL: cnt %= bits; return cnt ? ((x << cnt) | (x >> (bits - cnt))) & mk : x;
  default: cnt %= bits; return cnt ? ((x >> cnt) | (x << (bits - cnt))) & mk : x; /* XK_ROR */
  }
}

static u32 xlog2(u32 n) {
  u32 l = 0;
  while ((1u << l) < n) l++;
  return l;
}

/* The unmasked result of vector length vlb: a = the vvvv register, b = the
 * r/m operand (memory already broadcast where EVEX.b says so), old = the
 * destination before the instruction. */
static z512 xcompute(const xform *f, u32 vlb, const z512 *a, const z512 *b, const z512 *old, u8 imm) {
  const u32 es = f->es, n = vlb / es, bits = 8 * es, lanes = vlb / 16, per = 16 / es;
  z512 r;
  memset(r.b, 0, 64);
  switch (f->kind) {
  /* ---- A: element i of the result from element i of the sources */
  case XK_MINS: case XK_MAXS: case XK_MINU: case XK_MAXU: case XK_ABS: case XK_ADDS: case XK_ADDUS: case XK_SUBS:
  case XK_SUBUS: case XK_AVG: case XK_MULLO: case XK_MULHS: case XK_MULHU: case XK_MULUDQ: case XK_MULDQ:
    for (u32 i = 0; i < n; i++) {
      const u64 x = zget_el(a, i, es), y = zget_el(b, i, es);
      const i64 sx = (i64)sxn(x, (int)es), sy = (i64)sxn(y, (int)es);
      u64 v = 0;
      switch (f->kind) {
      case XK_MINS: v = (u64)(sx < sy ? sx : sy); break;
      case XK_MAXS: v = (u64)(sx > sy ? sx : sy); break;
      case XK_MINU: v = x < y ? x : y; break;
      case XK_MAXU: v = x > y ? x : y; break;
      case XK_ABS: v = sy < 0 ? 0 - y : y; break;
      case XK_ADDS: v = (u64)xsat_s(sx + sy, bits); break;  /* bytes and words only: no overflow in i64 */
      case XK_SUBS: v = (u64)xsat_s(sx - sy, bits); break;
      case XK_ADDUS: v = xsat_u((i64)(x + y), bits); break;
      case XK_SUBUS: v = xsat_u((i64)x - (i64)y, bits); break;
      case XK_AVG: v = (x + y + 1) >> 1; break;
      case XK_MULLO: v = x * y; break;                         /* the low half is the same signed or unsigned */
      case XK_MULHS: v = (u64)((sx * sy) >> 16); break;        /* words */
      case XK_MULHU: v = (x * y) >> 16; break;
      case XK_MULUDQ: v = (x & 0xffffffffu) * (y & 0xffffffffu); break;
      default: v = (u64)((i64)(int32_t)(u32)x * (i64)(int32_t)(u32)y); break; /* XK_MULDQ */
      }
      zput_el(&r, i, es, v);
    }
    break;
  /* ---- B */
  case XK_SRL: case XK_SRA: case XK_SLL: case XK_ROL: case XK_ROR:
    for (u32 i = 0; i < n; i++) {
      /* imm8: r/m shifted by the immediate; xmm: vvvv shifted by r/m's low qword; else by r/m's element i */
      const u64 x = f->cnt == XC_IMM ? zget_el(b, i, es) : zget_el(a, i, es);
      const u64 c = f->cnt == XC_IMM ? imm : f->cnt == XC_XMM ? zget_el(b, 0, 8) : zget_el(b, i, es);
      zput_el(&r, i, es, xshift(f->kind, x, c, bits));
    }
    break;
  case XK_BSRL: case XK_BSLL: { /* each 128-bit lane of r/m by imm8 bytes, 16 and more: zero */
    const u32 c = imm > 15 ? 16 : imm;
    for (u32 l = 0; l < lanes; l++)
      for (u32 j = 0; j < 16; j++) {
        if (f->kind == XK_BSRL) r.b[16 * l + j] = j + c < 16 ? b->b[16 * l + j + c] : 0;
        else r.b[16 * l + j] = j >= c ? b->b[16 * l + j - c] : 0;
      }
    break;
  }
  /* ---- C: within each 128-bit lane */
  case XK_SHUFB:
    for (u32 i = 0; i < vlb; i++) r.b[i] = (b->b[i] & 0x80) ? 0 : a->b[(i & ~15u) + (b->b[i] & 15)];
    break;
  case XK_SHUFD:
    for (u32 i = 0; i < n; i++) zput_el(&r, i, 4, zget_el(b, (i & ~3u) + ((imm >> (2 * (i & 3))) & 3), 4));
    break;
  case XK_SHUFHW: case XK_SHUFLW:
    for (u32 i = 0; i < n; i++) {
      const u32 q = i & 7, base = i & ~7u, half = f->kind == XK_SHUFHW ? 4 : 0;
      const u32 from = (q >= half && q < half + 4) ? base + half + ((imm >> (2 * (q & 3))) & 3) : i;
      zput_el(&r, i, 2, zget_el(b, from, 2));
    }
    break;
  case XK_UNPCKL: case XK_UNPCKH:
    for (u32 l = 0; l < lanes; l++)
      for (u32 j = 0; j < per; j++) {
        const u32 from = l * per + (f->kind == XK_UNPCKH ? per / 2 : 0) + j / 2;
        zput_el(&r, l * per + j, es, zget_el((j & 1) ? b : a, from, es));
      }
    break;
  case XK_PACKSS: case XK_PACKUS: { /* a lane's low half from vvvv's lane, its high half from r/m's */
    const u32 ss = f->ses, sper = 16 / ss;
    for (u32 l = 0; l < lanes; l++)
      for (u32 j = 0; j < per; j++) {
        const z512 *s = j < sper ? a : b;
        const i64 v = (i64)sxn(zget_el(s, l * sper + j % sper, ss), (int)ss);
        zput_el(&r, l * per + j, es, f->kind == XK_PACKSS ? (u64)xsat_s(v, bits) : xsat_u(v, bits));
      }
    break;
  }
  case XK_ALIGNR: /* (vvvv's lane : r/m's lane) >> imm8 bytes */
    for (u32 l = 0; l < lanes; l++)
      for (u32 j = 0; j < 16; j++) {
        const u32 k = j + imm;
        r.b[16 * l + j] = k < 16 ? b->b[16 * l + k] : k < 32 ? a->b[16 * l + k - 16] : 0;
      }
    break;
  /* ---- D: across lanes */
  case XK_PERM: /* indices in vvvv, the table in r/m */
    for (u32 i = 0; i < n; i++) zput_el(&r, i, es, zget_el(b, (u32)(zget_el(a, i, es) & (n - 1)), es));
    break;
  case XK_PERMQI:
    for (u32 i = 0; i < n; i++) zput_el(&r, i, 8, zget_el(b, (i & ~3u) + ((imm >> (2 * (i & 3))) & 3), 8));
    break;
  case XK_PERMI2: case XK_PERMT2: { /* i2: indices in the destination, tables vvvv : r/m; t2: indices in vvvv, tables destination : r/m */
    const z512 *idx = f->kind == XK_PERMI2 ? old : a, *t0 = f->kind == XK_PERMI2 ? a : old;
    const u32 lg = xlog2(n);
    for (u32 i = 0; i < n; i++) {
      const u64 ix = zget_el(idx, i, es);
      zput_el(&r, i, es, zget_el(((ix >> lg) & 1) ? b : t0, (u32)(ix & (n - 1)), es));
    }
    break;
  }
  case XK_VALIGN: { /* (vvvv : r/m) >> imm8 elements, the count modulo the element count */
    const u32 sh = imm & (n - 1);
    for (u32 i = 0; i < n; i++) zput_el(&r, i, es, i + sh < n ? zget_el(b, i + sh, es) : zget_el(a, i + sh - n, es));
    break;
  }
  case XK_SHUFI: /* the result's low half of lanes from vvvv, its high half from r/m */
    for (u32 l = 0; l < lanes; l++) {
      const u32 selbits = lanes == 4 ? 2 : 1;
      const u32 from = (imm >> (selbits * l)) & (lanes - 1);
      memcpy(r.b + 16 * l, (l < lanes / 2 ? a : b)->b + 16 * from, 16);
    }
    break;
  /* ---- E */
  case XK_MOVZX: case XK_MOVSX:
    for (u32 i = 0; i < n; i++) {
      const u64 x = zget_el(b, i, f->ses);
      zput_el(&r, i, es, f->kind == XK_MOVSX ? sxn(x, (int)f->ses) : x);
    }
    break;
  /* ---- F */
  case XK_INSERT:
    r = *a;
    memcpy(r.b + f->mfix * (imm & (vlb / f->mfix - 1)), b->b, f->mfix);
    break;
  case XK_EXTRACT: /* b here is the source register (ModRM.reg) */
    memcpy(r.b, b->b + f->mfix * (imm & (vlb / f->mfix - 1)), f->mfix);
    break;
  case XK_BCBLK:
    for (u32 o = 0; o < vlb; o += f->mfix) memcpy(r.b + o, b->b, f->mfix);
    break;
  default:
    break;
  }
  (void)old;
  return r;
}

static int exec_evexx(orc_machine *m, insn *d) {
  const u32 vv = d->vvvv;
  const int mem = d->is_mem;
  const xform f = xform_of(d->opmap, d->op, (int)d->vpp, d->vw, (int)(d->reg & 7));
  const int to_rm = f.kind == XK_EXTRACT || f.kind == XK_X2GPR || f.kind == XK_MOVQ_ST; /* r/m is the destination */
  int ud = f.kind == XK_NONE || f.kind == XK_BADDIGIT || d->ell == 3 || avx512_off(m);
  ud = ud || d->ell < f.minll || d->ell > f.maxll || (f.wreq >= 0 && (u32)f.wreq != d->vw);
  ud = ud || (f.shape == 2 && vv != 0) || (d->eb && (!mem || !f.bc));
  ud = ud || (d->ez && (!d->eaaa || (to_rm && mem))) || (f.nomask && d->eaaa);
  ud = ud || (f.memonly && !mem) || (f.regonly && mem);
  if (ud) {
    fault(m, WTFGPU_VEC_UD, 0);
    return X_FAULT;
  }
  if (m->r.cr0 & 8) {
    fault(m, 7, 0);
    return X_FAULT;
  }
  const u32 vlb = 16u << d->ell, es = f.es;
  const u8 imm = d->bytes[d->len - 1];

  /* ---- G, H: no opmask, their own operands */
  switch (f.kind) {
  case XK_M2V: {
    z512 r;
    memset(r.b, 0, 64);
    for (u32 i = 0; i < vlb / es; i++)
      if ((m->r.k[d->rm & 7] >> i) & 1) zput_el(&r, i, es, ~0ULL);
    zput(m, d->reg, r, vlb);
    return X_OK;
  }
  case XK_V2M: {
    const z512 s = zreg(m, d->rm);
    u64 kv = 0;
    for (u32 i = 0; i < vlb / es; i++) kv |= ((zget_el(&s, i, es) >> (8 * es - 1)) & 1) << i;
    m->r.k[d->reg & 7] = kv;
    return X_OK;
  }
  case XK_GPR2X: case XK_MOVQ_LD: { /* xmm = the operand zero-extended */
    z512 r;
    memset(r.b, 0, 64);
    if (mem) {
      if (vread(m, d->ea, es, r.b)) return X_FAULT;
    } else if (f.kind == XK_GPR2X) {
      zput_el(&r, 0, es, m->r.gpr[d->rm & 15]);
    } else {
      const z512 s = zreg(m, d->rm);
      memcpy(r.b, s.b, 8);
    }
    zput(m, d->reg, r, 16);
    return X_OK;
  }
  case XK_X2GPR: case XK_MOVQ_ST: {
    const z512 s = zreg(m, d->reg);
    if (mem) return vwrite(m, d->ea, es, s.b) ? X_FAULT : X_OK;
    if (f.kind == XK_X2GPR) {
      m->r.gpr[d->rm & 15] = zget_el(&s, 0, es); /* vmovd r32: zero-extended to 64 bits */
    } else {
      z512 r;
      memset(r.b, 0, 64);
      memcpy(r.b, s.b, 8);
      zput(m, d->rm, r, 16);
    }
    return X_OK;
  }
  default:
    break;
  }

  /* the elements the opmask counts: the destination's (vextracti: the block's) */
  const u32 dlb = f.kind == XK_EXTRACT ? f.mfix : vlb, n = dlb / es;
  const u64 all = xmask_bits(n);
  const u64 selm = d->eaaa ? (m->r.k[d->eaaa] & all) : all;

  if (f.kind == XK_EXTRACT) {
    const z512 s = zreg(m, d->reg), none = s;
    const z512 r = xcompute(&f, vlb, &none, &s, &none, imm);
    if (mem) { /* exception class E6NF: the whole block is checked, whatever the mask; selected elements are written */
      u64 pa[2];
      u32 nn[2];
      if (vprobe(m, d->ea, dlb, ACC_W, pa, nn)) return X_FAULT;
      return zmem_store(m, d->ea, es, n, selm, d->eaaa != 0, &r) ? X_FAULT : X_OK;
    }
    z512 out = zreg(m, d->rm);
    for (u32 i = 0; i < n; i++)
      zput_el(&out, i, es, ((selm >> i) & 1) ? zget_el(&r, i, es) : d->ez ? 0 : zget_el(&out, i, es));
    zput(m, d->rm, out, dlb);
    return X_OK;
  }

  /* ---- the r/m source */
  z512 src;
  memset(src.b, 0, 64);
  if (mem) {
    if (d->eb) { /* one element, repeated; not read when no element is selected (a form that reads whole: always) */
      const u32 reps = 64 / f.bc;
      if (zmem_load(m, d->ea, f.bc, 1, (selm || f.whole) ? 1 : 0, &src)) return X_FAULT;
      for (u32 i = 1; i < reps; i++) zput_el(&src, i, f.bc, zget_el(&src, 0, f.bc));
    } else if (f.whole) {
      const u32 sz = xf_msize(&f, vlb);
      if (zmem_load(m, d->ea, 1, sz, xmask_bits(sz), &src)) return X_FAULT;
    } else if (f.kind == XK_BCBLK) { /* source element j feeds destination elements j, j + cnt, ... */
      const u32 cnt = f.mfix / es;
      u64 need = 0;
      for (u32 i = 0; i < n; i++)
        if ((selm >> i) & 1) need |= 1ULL << (i % cnt);
      if (zmem_load(m, d->ea, es, cnt, need, &src)) return X_FAULT;
    } else { /* element i of the operand feeds element i of the result alone */
      if (zmem_load(m, d->ea, f.ses, n, selm, &src)) return X_FAULT;
    }
  } else {
    src = zreg(m, d->rm);
  }
  const u32 dreg = f.shape == 1 ? vv : d->reg;
  const z512 a = zreg(m, vv), old = zreg(m, dreg);
  const z512 r = xcompute(&f, vlb, &a, &src, &old, imm);
  z512 out = old;
  for (u32 i = 0; i < n; i++)
    zput_el(&out, i, es, ((selm >> i) & 1) ? zget_el(&r, i, es) : d->ez ? 0 : zget_el(&old, i, es));
  zput(m, dreg, out, vlb);
  return X_OK;
}
