// engine_avx512.h — the AVX-512 subset: EVEX-encoded moves,
// logic, add / sub, unsigned min / max, compares and tests into opmask
// registers, vpternlog and broadcasts at 128 / 256 / 512 bits with merging or
// zeroing masks, and the VEX-encoded opmask instructions (kmov, kortest,
// ktest, kadd, kunpck, the k logic and shifts) — what vectorised memcpy / memset / strlen /
// memchr / strcmp paths built for AVX-512 run — and the integer forms of U49
// (engine_avx512x.h, evexx_exec): element-wise arithmetic (signed / unsigned
// min / max, abs, saturating add / sub, avg, the multiplies), shifts and
// rotates by imm8, by an xmm count and per element, vpslldq / vpsrldq, the
// in-lane shuffles (vpshufb / d / hw / lw, vpunpck*, vpack*, vpalignr), the
// cross-lane permutes (vpermb / w / d / q, vpermi2* / vpermt2*, valignd / q,
// vshufi32x4 / 64x2), the widening loads vpmovzx* / vpmovsx*, and (evexm_exec)
// the 128- / 256-bit block inserts / extracts / broadcasts, the mask <->
// vector moves vpmovm2* / vpmov*2m and vmovd / vmovq. A form runs whether or
// not CPUID leaf 7 names its extension (the DQ / VBMI variants differ from an
// F / BW form only in W; a snapshot's guest chose its code paths on the
// capture host). Every other EVEX encoding is UNIMPLEMENTED (U36): floating
// point, the down-converts, compress / expand, gathers / scatters, vpconflict
// / vplzcnt, vpmaddwd / vpsadbw / vpmaddubsw, vpextr / vpinsr, IFMA / VNNI /
// BITALG / VPOPCNTDQ / FP16. The state (zmm0-31, k0-7) lives in the lane's cold
// state (wtfgpu_regs_t: xmm / ymmh / zmmh for zmm0-15, zmm_hi for 16-31, k).
//
// Memory: an element whose mask bit is 0 is neither read nor written, so it
// cannot fault (memory fault suppression); every page is checked before
// anything is written; the aligned forms need VL alignment unless every
// element is masked off. A load's fault is reported at the first selected
// byte that faults; a masked store's at its lowest selected element's first
// byte or else its highest one's last byte (what native execution reports). Faults are raised in the order #UD, #NM, #GP
// (alignment), then the memory access, as the VEX forms do (U23).
#pragma once

namespace wtfgpu_dev {

// UOp::opreg of an EVEX op: O_SSE's VEX fields (bit 0 set, bit 2 W, bits 4-7
// vvvv[3:0], bits 8-12 the map, bit 16 a prefix before it) plus bit 17 EVEX,
// bits 18-19 L'L, bit 21 z, bit 22 b, bits 23-25 aaa, bit 26 V' (vvvv[4]);
// bit 27 carries R' through decode only; bit 28 marks a U49 form (evexx_exec),
// with bit 29 its block / mask / GPR moves (evexm_exec).
// Bit 20 is kMmxForm (engine_sse.h) and stays outside the EVEX fields.
// UOp::reg and UOp::rm carry the 5-bit register numbers (R' and X included).
constexpr u32 EVX = 1u << 17;
constexpr u32 EVXX = 1u << 28;
constexpr u32 EVXM = 1u << 29;
static_assert(kMmxForm == (1u << 20) && !(kMmxForm & (EVX | EVXX | EVXM | (3u << 18) | (0x7fu << 21))),
              "kMmxForm must stay outside the EVEX fields of UOp::opreg");
__host__ __device__ inline u32 evex_ll(u32 x) { return (x >> 18) & 3; }
__host__ __device__ inline u32 evex_vvvv(u32 x) { return ((x >> 4) & 15) | (((x >> 26) & 1) << 4); }

enum : u32 {
  EZ_NONE = 0, EZ_MOV, EZ_LOGIC, EZ_ADD, EZ_SUB, EZ_MINU, EZ_MAXU, EZ_CMPEQ, EZ_CMPGT, EZ_CMP, EZ_TESTM,
  EZ_TERN, EZ_BCAST, EZ_BCASTR,
  EZ_WUD = 15,  // #UD at decode (native execution): the opcode is in the subset, this W or /digit is not
  // U49 (engine_avx512x.h): kinds from EZ_X on run in evexx_exec
  EZ_X = 16, EZ_BIN = EZ_X, EZ_UN, EZ_SHI, EZ_SHX, EZ_BSH, EZ_PSHUFB, EZ_PSHUFD, EZ_PSHUFW, EZ_UNPCK, EZ_PACK,
  EZ_ALIGNR, EZ_PERM, EZ_PERMQI, EZ_PERMI2, EZ_PERMT2, EZ_VALIGN, EZ_SHUFI, EZ_PMOVX,
  // kinds from EZ_Y on run in evexm_exec: 128- / 256-bit block insert, extract and broadcast, mask <-> vector,
  // vmovd / vmovq
  EZ_Y = 40, EZ_INS = EZ_Y, EZ_EXT, EZ_BCB, EZ_M2V, EZ_V2M, EZ_GMOV
};
// EZ_BIN's sub
enum : u32 {
  XB_MINS = 0, XB_MAXS, XB_MINU, XB_MAXU, XB_ADDS, XB_ADDUS, XB_SUBS, XB_SUBUS, XB_AVG, XB_MULL, XB_MULH, XB_MULHU,
  XB_MULUDQ, XB_MULDQ, XB_SLLV, XB_SRLV, XB_SRAV, XB_ROLV, XB_RORV
};
// the shifts' sub (EZ_SHI / EZ_SHX): XS_ROR / XS_ROL by imm8 only
enum : u32 { XS_SRL = 0, XS_SRA, XS_SLL, XS_ROR, XS_ROL };
// The memory operand's size class: what disp8 scales by (SDM 2.7.5) and how
// many bytes the operand has. MC_FULL: the vector, or one element under
// EVEX.b; MC_FULLMEM: the vector, no broadcast (the byte / word forms);
// MC_HALF / QUARTER / EIGHTH: that part of the vector (vpmovzx / sx);
// MC_M128: 16 bytes at every length (the shifts' xmm count); MC_T8 / T16 /
// T32: the 8- / 16- / 32-byte tuples of the block forms; MC_T1S: one scalar
// of the element size (vmovd / vmovq).
enum : u32 { MC_FULL = 0, MC_FULLMEM, MC_HALF, MC_QUARTER, MC_EIGHTH, MC_M128, MC_T8, MC_T16, MC_T32, MC_T1S };
enum : u32 {
  XF_IMM = 1, XF_TWO = 2, XF_VDST = 4, XF_NOMASK = 8, XF_NF = 16, XF_NO128 = 32, XF_ONLY512 = 64, XF_ONLY128 = 128,
  XF_MEMONLY = 256, XF_REGONLY = 512
};
struct EForm {
  u32 kind, es, sub;  // sub: logic op (0 and 1 andn 2 or 3 xor), cmp signedness (1 signed), testm negation
  bool store, aligned, bcastok, kdest;
  bool nt = false;    // the non-temporal moves: memory operand only, no masking (aaa != 0: #UD)
  // U49
  u32 mc = MC_FULL;
  u32 ses = 0;        // the source's element (vpmovzx / sx, the packs): also what EVEX.b broadcasts; the block
                      // forms' block bytes
  u32 fl = 0;         // XF_IMM an imm8 follows; XF_TWO no vvvv operand; XF_VDST the destination is vvvv (ModRM.reg
                      // a /digit); XF_NOMASK aaa != 0 is #UD; XF_NF a masked-off element of a memory source is
                      // still read (no fault suppression); XF_NO128 no 128-bit form; XF_ONLY512 / XF_ONLY128
                      // that length alone; XF_MEMONLY / XF_REGONLY no register / memory r/m operand
};
__host__ __device__ inline EForm xform(u32 kind, u32 es, u32 sub, bool bc, u32 fl = 0, u32 mc = MC_FULL, u32 ses = 0) {
  EForm f{kind, es, sub, false, false, bc, false};
  f.mc = (mc == MC_FULL && !bc) ? (u32)MC_FULLMEM : mc;
  f.ses = ses ? ses : es;
  f.fl = fl;
  return f;
}

// The subset, by (map, opcode, pp, W). pp: 0 none, 1 66, 2 f3, 3 f2.
// digit: ModRM.reg[2:0], which selects the form of the groups 0f 71 / 72 / 73.
__host__ __device__ inline EForm evex_form(u32 map, u32 c, u32 pp, u32 w, u32 digit = 0) {
  EForm f{EZ_NONE, 0, 0, false, false, false, false};
  const EForm wud{EZ_WUD, 0, 0, false, false, false, false};  // a U49 opcode at a W or /digit it does not have
  const u32 wes = w ? 8u : 4u;
  if (map == 1) {
    if ((c == 0x10 || c == 0x11 || c == 0x28 || c == 0x29) && pp <= 1 && w == pp)  // vmovups/upd, vmovaps/apd
      return EForm{EZ_MOV, pp ? 8u : 4u, 0, (c & 1) != 0, c >= 0x28, false, false};
    if ((c == 0x2b && pp <= 1 && w == pp) || (c == 0xe7 && pp == 1 && !w))  // vmovntps / pd, vmovntdq
      return EForm{EZ_MOV, c == 0x2b && pp ? 8u : 4u, 0, true, true, false, false, true};
    if (c == 0x6f || c == 0x7f) {
      if (pp == 1) return EForm{EZ_MOV, w ? 8u : 4u, 0, c == 0x7f, true, false, false};   // vmovdqa32 / 64
      if (pp == 2) return EForm{EZ_MOV, w ? 8u : 4u, 0, c == 0x7f, false, false, false};  // vmovdqu32 / 64
      if (pp == 3) return EForm{EZ_MOV, w ? 2u : 1u, 0, c == 0x7f, false, false, false};  // vmovdqu8 / 16
      return f;
    }
    if (c == 0x70) {  // vpshufd / vpshufhw / vpshuflw
      if (pp == 1) return w ? wud : xform(EZ_PSHUFD, 4, 0, true, XF_IMM | XF_TWO | XF_NF);
      if (pp == 2 || pp == 3) return xform(EZ_PSHUFW, 2, pp == 2 ? 1 : 0, false, XF_IMM | XF_TWO | XF_NF);
      return f;
    }
    // vmovd / vmovq (128 bits, no mask): sub 0 xmm <- r/m32 / 64, 1 r/m32 / 64 <- xmm, 2 xmm <- xmm / m64, 3 xmm / m64 <- xmm
    if (c == 0x6e && pp == 1) return xform(EZ_GMOV, wes, 0, false, XF_TWO | XF_NOMASK | XF_ONLY128, MC_T1S);
    if (c == 0x7e && pp == 1) return xform(EZ_GMOV, wes, 1, false, XF_TWO | XF_NOMASK | XF_ONLY128, MC_T1S);
    if (c == 0x7e && pp == 2) return w ? xform(EZ_GMOV, 8, 2, false, XF_TWO | XF_NOMASK | XF_ONLY128, MC_T1S) : wud;
    if (c == 0xd6 && pp == 1) return w ? xform(EZ_GMOV, 8, 3, false, XF_TWO | XF_NOMASK | XF_ONLY128, MC_T1S) : wud;
    if (pp != 1) return f;
    switch (c) {
      case 0x60: return xform(EZ_UNPCK, 1, 0, false, XF_NF);
      case 0x61: return xform(EZ_UNPCK, 2, 0, false, XF_NF);
      case 0x62: return w ? wud : xform(EZ_UNPCK, 4, 0, true, XF_NF);
      case 0x6c: return w ? xform(EZ_UNPCK, 8, 0, true, XF_NF) : wud;
      case 0x68: return xform(EZ_UNPCK, 1, 1, false, XF_NF);
      case 0x69: return xform(EZ_UNPCK, 2, 1, false, XF_NF);
      case 0x6a: return w ? wud : xform(EZ_UNPCK, 4, 1, true, XF_NF);
      case 0x6d: return w ? xform(EZ_UNPCK, 8, 1, true, XF_NF) : wud;
      case 0x63: return xform(EZ_PACK, 1, 0, false, XF_NF, MC_FULL, 2);  // vpacksswb
      case 0x67: return xform(EZ_PACK, 1, 1, false, XF_NF, MC_FULL, 2);  // vpackuswb
      case 0x6b: return w ? wud : xform(EZ_PACK, 2, 0, true, XF_NF, MC_FULL, 4);  // vpackssdw
      case 0x71:  // vpsrlw / vpsraw / vpsllw by imm8
        if (digit == 2 || digit == 4 || digit == 6)
          return xform(EZ_SHI, 2, digit == 2 ? XS_SRL : digit == 4 ? XS_SRA : XS_SLL, false, XF_IMM | XF_VDST);
        return wud;
      case 0x72:  // vprord / q, vprold / q, vpsrld, vpsrad / q, vpslld
        if (digit == 0 || digit == 1) return xform(EZ_SHI, wes, digit ? XS_ROL : XS_ROR, true, XF_IMM | XF_VDST);
        if (digit == 4) return xform(EZ_SHI, wes, XS_SRA, true, XF_IMM | XF_VDST);
        if ((digit == 2 || digit == 6) && !w) return xform(EZ_SHI, 4, digit == 2 ? XS_SRL : XS_SLL, true, XF_IMM | XF_VDST);
        return wud;
      case 0x73:  // vpsrlq, vpsrldq, vpsllq, vpslldq
        if ((digit == 2 || digit == 6) && w) return xform(EZ_SHI, 8, digit == 2 ? XS_SRL : XS_SLL, true, XF_IMM | XF_VDST);
        if (digit == 3 || digit == 7) return xform(EZ_BSH, 1, digit == 7, false, XF_IMM | XF_VDST | XF_NOMASK | XF_NF);
        return wud;
      case 0xd1: return xform(EZ_SHX, 2, XS_SRL, false, XF_NF, MC_M128);
      case 0xd2: return w ? wud : xform(EZ_SHX, 4, XS_SRL, false, XF_NF, MC_M128);
      case 0xd3: return w ? xform(EZ_SHX, 8, XS_SRL, false, XF_NF, MC_M128) : wud;
      case 0xe1: return xform(EZ_SHX, 2, XS_SRA, false, XF_NF, MC_M128);
      case 0xe2: return xform(EZ_SHX, wes, XS_SRA, false, XF_NF, MC_M128);
      case 0xf1: return xform(EZ_SHX, 2, XS_SLL, false, XF_NF, MC_M128);
      case 0xf2: return w ? wud : xform(EZ_SHX, 4, XS_SLL, false, XF_NF, MC_M128);
      case 0xf3: return w ? xform(EZ_SHX, 8, XS_SLL, false, XF_NF, MC_M128) : wud;
      case 0xd5: return xform(EZ_BIN, 2, XB_MULL, false);
      case 0xe4: return xform(EZ_BIN, 2, XB_MULHU, false);
      case 0xe5: return xform(EZ_BIN, 2, XB_MULH, false);
      case 0xd8: return xform(EZ_BIN, 1, XB_SUBUS, false);
      case 0xd9: return xform(EZ_BIN, 2, XB_SUBUS, false);
      case 0xdc: return xform(EZ_BIN, 1, XB_ADDUS, false);
      case 0xdd: return xform(EZ_BIN, 2, XB_ADDUS, false);
      case 0xe8: return xform(EZ_BIN, 1, XB_SUBS, false);
      case 0xe9: return xform(EZ_BIN, 2, XB_SUBS, false);
      case 0xec: return xform(EZ_BIN, 1, XB_ADDS, false);
      case 0xed: return xform(EZ_BIN, 2, XB_ADDS, false);
      case 0xe0: return xform(EZ_BIN, 1, XB_AVG, false);
      case 0xe3: return xform(EZ_BIN, 2, XB_AVG, false);
      case 0xea: return xform(EZ_BIN, 2, XB_MINS, false);
      case 0xee: return xform(EZ_BIN, 2, XB_MAXS, false);
      case 0xf4: return w ? xform(EZ_BIN, 8, XB_MULUDQ, true) : wud;
      case 0xdb: return EForm{EZ_LOGIC, w ? 8u : 4u, 0, false, false, true, false};
      case 0xdf: return EForm{EZ_LOGIC, w ? 8u : 4u, 1, false, false, true, false};
      case 0xeb: return EForm{EZ_LOGIC, w ? 8u : 4u, 2, false, false, true, false};
      case 0xef: return EForm{EZ_LOGIC, w ? 8u : 4u, 3, false, false, true, false};
      case 0xfc: return EForm{EZ_ADD, 1, 0, false, false, false, false};
      case 0xfd: return EForm{EZ_ADD, 2, 0, false, false, false, false};
      case 0xfe: return w ? f : EForm{EZ_ADD, 4, 0, false, false, true, false};
      case 0xd4: return w ? EForm{EZ_ADD, 8, 0, false, false, true, false} : f;
      case 0xf8: return EForm{EZ_SUB, 1, 0, false, false, false, false};
      case 0xf9: return EForm{EZ_SUB, 2, 0, false, false, false, false};
      case 0xfa: return w ? f : EForm{EZ_SUB, 4, 0, false, false, true, false};
      case 0xfb: return w ? EForm{EZ_SUB, 8, 0, false, false, true, false} : f;
      case 0xda: return EForm{EZ_MINU, 1, 0, false, false, false, false};
      case 0xde: return EForm{EZ_MAXU, 1, 0, false, false, false, false};
      case 0x74: return EForm{EZ_CMPEQ, 1, 0, false, false, false, true};
      case 0x75: return EForm{EZ_CMPEQ, 2, 0, false, false, false, true};
      case 0x76: return w ? f : EForm{EZ_CMPEQ, 4, 0, false, false, true, true};
      case 0x64: return EForm{EZ_CMPGT, 1, 0, false, false, false, true};
      case 0x65: return EForm{EZ_CMPGT, 2, 0, false, false, false, true};
      case 0x66: return w ? f : EForm{EZ_CMPGT, 4, 0, false, false, true, true};
      default: return f;
    }
  }
  if (map == 2) {
    if ((c == 0x26 || c == 0x27) && (pp == 1 || pp == 2))  // vptestm / vptestnm b w (26), d q (27)
      return EForm{EZ_TESTM, c == 0x26 ? (w ? 2u : 1u) : (w ? 8u : 4u), pp == 2 ? 1u : 0u, false, false, c == 0x27,
                   true};
    if (pp == 2) {  // vpmovm2 b w d q, vpmov b w d q 2m (no mask, registers only)
      if (c == 0x28 || c == 0x38) return xform(EZ_M2V, c == 0x28 ? (w ? 2u : 1u) : wes, 0, false, XF_TWO | XF_NOMASK | XF_REGONLY);
      if (c == 0x29 || c == 0x39) return xform(EZ_V2M, c == 0x29 ? (w ? 2u : 1u) : wes, 0, false, XF_TWO | XF_NOMASK | XF_REGONLY);
    }
    if (pp != 1) return f;
    if (c == 0x59 && !w) return xform(EZ_BCB, 4, 0, false, XF_TWO, MC_T8, 8);                      // vbroadcasti32x2
    if (c == 0x5a) return xform(EZ_BCB, wes, 0, false, XF_TWO | XF_NO128 | XF_MEMONLY, MC_T16, 16);    // 32x4 / 64x2
    if (c == 0x5b) return xform(EZ_BCB, wes, 0, false, XF_TWO | XF_ONLY512 | XF_MEMONLY, MC_T32, 32);  // 32x8 / 64x4
    if ((c >= 0x20 && c <= 0x25) || (c >= 0x30 && c <= 0x35)) {  // vpmovsx / vpmovzx bw bd bq wd wq dq
      const u32 t = c & 15, sgn = c < 0x30;
      if (t == 5 && w) return wud;
      const u32 des = t == 0 ? 2u : (t == 1 || t == 3) ? 4u : 8u, ses = t < 3 ? 1u : t < 5 ? 2u : 4u;
      return xform(EZ_PMOVX, des, sgn, false, XF_TWO, des / ses == 2 ? MC_HALF : des / ses == 4 ? MC_QUARTER : MC_EIGHTH,
                   ses);
    }
    switch (c) {
      case 0x00: return xform(EZ_PSHUFB, 1, 0, false, XF_NF);
      case 0x1c: return xform(EZ_UN, 1, 0, false, XF_TWO);
      case 0x1d: return xform(EZ_UN, 2, 0, false, XF_TWO);
      case 0x1e: return w ? wud : xform(EZ_UN, 4, 0, true, XF_TWO);
      case 0x1f: return w ? xform(EZ_UN, 8, 0, true, XF_TWO) : wud;
      case 0x28: return w ? xform(EZ_BIN, 8, XB_MULDQ, true) : wud;
      case 0x2b: return w ? wud : xform(EZ_PACK, 2, 1, true, XF_NF, MC_FULL, 4);  // vpackusdw
      case 0x38: return xform(EZ_BIN, 1, XB_MINS, false);
      case 0x39: return xform(EZ_BIN, wes, XB_MINS, true);
      case 0x3b: return xform(EZ_BIN, wes, XB_MINU, true);
      case 0x3c: return xform(EZ_BIN, 1, XB_MAXS, false);
      case 0x3d: return xform(EZ_BIN, wes, XB_MAXS, true);
      case 0x3f: return xform(EZ_BIN, wes, XB_MAXU, true);
      case 0x40: return xform(EZ_BIN, wes, XB_MULL, true);
      case 0x10: return w ? xform(EZ_BIN, 2, XB_SRLV, false) : wud;
      case 0x11: return w ? xform(EZ_BIN, 2, XB_SRAV, false) : wud;
      case 0x12: return w ? xform(EZ_BIN, 2, XB_SLLV, false) : wud;
      case 0x45: return xform(EZ_BIN, wes, XB_SRLV, true);
      case 0x46: return xform(EZ_BIN, wes, XB_SRAV, true);
      case 0x47: return xform(EZ_BIN, wes, XB_SLLV, true);
      case 0x14: return xform(EZ_BIN, wes, XB_RORV, true);
      case 0x15: return xform(EZ_BIN, wes, XB_ROLV, true);
      case 0x36: return xform(EZ_PERM, wes, 0, true, XF_NF | XF_NO128);
      case 0x8d: return xform(EZ_PERM, w ? 2 : 1, 0, false, XF_NF);
      case 0x75: return xform(EZ_PERMI2, w ? 2 : 1, 0, false, XF_NF);
      case 0x76: return xform(EZ_PERMI2, wes, 0, true, XF_NF);
      case 0x7d: return xform(EZ_PERMT2, w ? 2 : 1, 0, false, XF_NF);
      case 0x7e: return xform(EZ_PERMT2, wes, 0, true, XF_NF);
      case 0x2a: return w ? f : EForm{EZ_MOV, 4, 0, false, true, false, false, true};  // vmovntdqa
      case 0x29: return w ? EForm{EZ_CMPEQ, 8, 0, false, false, true, true} : f;
      case 0x37: return w ? EForm{EZ_CMPGT, 8, 0, false, false, true, true} : f;
      case 0x3a: return EForm{EZ_MINU, 2, 0, false, false, false, false};
      case 0x3e: return EForm{EZ_MAXU, 2, 0, false, false, false, false};
      case 0x78: return w ? f : EForm{EZ_BCAST, 1, 0, false, false, false, false};
      case 0x79: return w ? f : EForm{EZ_BCAST, 2, 0, false, false, false, false};
      case 0x58: return w ? f : EForm{EZ_BCAST, 4, 0, false, false, false, false};
      case 0x59: return w ? EForm{EZ_BCAST, 8, 0, false, false, false, false} : f;
      case 0x7a: return w ? f : EForm{EZ_BCASTR, 1, 0, false, false, false, false};
      case 0x7b: return w ? f : EForm{EZ_BCASTR, 2, 0, false, false, false, false};
      case 0x7c: return EForm{EZ_BCASTR, w ? 8u : 4u, 0, false, false, false, false};
      default: return f;
    }
  }
  if (map == 3 && pp == 1) {
    // vinserti / vextracti 32x4, 64x2 (16-byte blocks; 256 and 512 bits) and 32x8, 64x4 (32-byte blocks; 512 bits)
    if (c == 0x38) return xform(EZ_INS, wes, 0, false, XF_IMM | XF_NF | XF_NO128, MC_T16, 16);
    if (c == 0x3a) return xform(EZ_INS, wes, 0, false, XF_IMM | XF_NF | XF_ONLY512, MC_T32, 32);
    if (c == 0x39) return xform(EZ_EXT, wes, 0, false, XF_IMM | XF_TWO | XF_NO128, MC_T16, 16);
    if (c == 0x3b) return xform(EZ_EXT, wes, 0, false, XF_IMM | XF_TWO | XF_ONLY512, MC_T32, 32);
    if (c == 0x0f) return xform(EZ_ALIGNR, 1, 0, false, XF_IMM | XF_NF);
    if (c == 0x00) return w ? xform(EZ_PERMQI, 8, 0, true, XF_IMM | XF_TWO | XF_NF | XF_NO128) : wud;
    if (c == 0x03) return xform(EZ_VALIGN, wes, 0, true, XF_IMM | XF_NF);
    if (c == 0x43) return xform(EZ_SHUFI, wes, 0, true, XF_IMM | XF_NF | XF_NO128);
    if (c == 0x25) return EForm{EZ_TERN, w ? 8u : 4u, 0, false, false, true, false};
    if (c == 0x3e || c == 0x3f) return EForm{EZ_CMP, w ? 2u : 1u, c & 1, false, false, false, true};
    if (c == 0x1e || c == 0x1f) return EForm{EZ_CMP, w ? 8u : 4u, c & 1, false, false, true, true};
  }
  return f;
}

// disp8 * N (SDM 2.7.5): by the memory operand's size class — the vector
// length (full / full-mem), a half / quarter / eighth of it, 16 bytes — or,
// for a broadcast memory operand (EVEX.b, or the broadcast instructions'
// element), the element size. vl: 16 / 32 / 64.
__host__ __device__ inline u32 evex_disp8_n(const EForm &f, u32 vl, u32 b) {
  if (f.kind == EZ_BCAST) return f.es;
  if (b && f.bcastok) return f.kind >= EZ_X ? f.ses : f.es;
  switch (f.mc) {
    case MC_HALF: return vl / 2;
    case MC_QUARTER: return vl / 4;
    case MC_EIGHTH: return vl / 8;
    case MC_M128: return 16;
    case MC_T8: return 8;
    case MC_T16: return 16;
    case MC_T32: return 32;
    case MC_T1S: return f.es;
    default: return vl;
  }
}

// The VEX-encoded opmask instructions (0f 41-47 / 90-93 / 98 / 99, 0f 3a
// 30-33): operand bits (8 / 16 / 32 / 64), 0 = not one of them.
__host__ __device__ inline u32 kop_bits(u32 map, u32 c, u32 pp, u32 w) {
  if (map == 3) return (c >= 0x30 && c <= 0x33 && pp == 1) ? ((c & 1) ? (w ? 64u : 32u) : (w ? 16u : 8u)) : 0u;
  if (map != 1) return 0;
  const bool grp = (c >= 0x41 && c <= 0x47 && c != 0x43) || c == 0x4a || c == 0x90 || c == 0x91 || c == 0x98 ||
                   c == 0x99;
  if (grp) return pp == 0 ? (w ? 64u : 16u) : pp == 1 ? (w ? 32u : 8u) : 0u;
  if (c == 0x4b) return pp == 1 ? (w ? 0u : 16u) : pp == 0 ? (w ? 64u : 32u) : 0u;  // kunpckbw / wd / dq: result bits
  if (c == 0x92 || c == 0x93) return pp == 0 ? (w ? 0u : 16u) : pp == 1 ? (w ? 0u : 8u) : pp == 3 ? (w ? 64u : 32u) : 0u;
  return 0;
}

struct Z512 {
  u64 q[8];
};
__device__ __forceinline__ Z512 zmm_get(const Dev &P, const Lane &L, u32 r) {
  const wtfgpu_regs_t &F = P.full[L.lane];
  Z512 v;
  if (r < 16) {
    v.q[0] = F.xmm[r][0], v.q[1] = F.xmm[r][1], v.q[2] = F.ymmh[r][0], v.q[3] = F.ymmh[r][1];
    for (u32 i = 0; i < 4; i++) v.q[4 + i] = F.zmmh[r][i];
  } else {
    for (u32 i = 0; i < 8; i++) v.q[i] = F.zmm_hi[r - 16][i];
  }
  return v;
}
// an EVEX destination: the bits above the vector length zeroed
__device__ __forceinline__ void zmm_put(const Dev &P, const Lane &L, u32 r, Z512 v, u32 vl) {
  wtfgpu_regs_t &F = P.full[L.lane];
  for (u32 i = vl / 8; i < 8; i++) v.q[i] = 0;
  if (r < 16) {
    F.xmm[r][0] = v.q[0], F.xmm[r][1] = v.q[1], F.ymmh[r][0] = v.q[2], F.ymmh[r][1] = v.q[3];
    for (u32 i = 0; i < 4; i++) F.zmmh[r][i] = v.q[4 + i];
  } else {
    for (u32 i = 0; i < 8; i++) F.zmm_hi[r - 16][i] = v.q[i];
  }
}
__device__ __forceinline__ u64 zel(const Z512 &v, u32 i, u32 w) {
  const u32 bit = i * w * 8;
  return (v.q[bit >> 6] >> (bit & 63)) & szmask(w);
}
__device__ __forceinline__ void zset(Z512 &v, u32 i, u32 w, u64 x) {
  const u32 bit = i * w * 8, s = bit & 63;
  const u64 mk = szmask(w) << s;
  v.q[bit >> 6] = (v.q[bit >> 6] & ~mk) | ((x << s) & mk);
}
__device__ __forceinline__ u64 kmask_bits(u32 n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

// The selected elements of an n-element operand at ea (es bytes each): every
// page checked first (loads: the selected elements' pages), then the moves.
__device__ __forceinline__ bool zspan(Lane &L, u64 ea, u32 es, u32 n, u64 sel, int acc) {
  if (sel == kmask_bits(n)) return span_ok(L, ea, es * n, acc);
  for (u32 i = 0; i < n; i++)
    if (((sel >> i) & 1) && !span_ok(L, ea + (u64)i * es, es, acc)) return false;
  return true;
}
__device__ __forceinline__ bool zload(Lane &L, u64 ea, u32 es, u32 n, u64 sel, Z512 &v) {
  for (u32 i = 0; i < 8; i++) v.q[i] = 0;
  if (!sel) return true;
  tn_mute(L.lane);  // Tenet: one access of the operand
  bool ok = zspan(L, ea, es, n, sel, ACC_R);
  if (ok && sel == kmask_bits(n) && es * n >= 8) {
    for (u32 i = 0; ok && i < es * n / 8; i++) ok = vread(L, ea + 8 * i, 8, v.q[i]);
  } else {
    for (u32 i = 0; ok && i < n; i++) {
      u64 x = 0;
      if ((sel >> i) & 1) ok = vread(L, ea + (u64)i * es, es, x);
      zset(v, i, es, x);
    }
  }
  return tn_unmute(L.lane, ea, es * n, TN_R, ok);
}
// A masked store (aaa != 0) checks two bytes, as the hardware reports them:
// the lowest selected element's first byte, then the highest one's last byte
// (native vectors: a fault on the upper page is reported at that last byte).
__device__ __forceinline__ bool zstore(Lane &L, u64 ea, u32 es, u32 n, u64 sel, bool masked, const Z512 &v) {
  if (!sel) return true;
  if (masked) {
    const u32 lo = __builtin_ctzll(sel), hi = 63 - __builtin_clzll(sel);
    if (!xlate(L, ea + (u64)lo * es, ACC_WPROBE) || !xlate(L, ea + (u64)hi * es + es - 1, ACC_WPROBE)) return false;
  } else if (!zspan(L, ea, es, n, sel, ACC_WPROBE)) {
    return false;
  }
  tn_mute(L.lane);
  bool ok = true;
  if (sel == kmask_bits(n) && es * n >= 8) {
    for (u32 i = 0; ok && i < es * n / 8; i++) ok = vwrite(L, ea + 8 * i, 8, v.q[i]);
  } else {
    for (u32 i = 0; ok && i < n; i++)
      if ((sel >> i) & 1) ok = vwrite(L, ea + (u64)i * es, es, zel(v, i, es));
  }
  return tn_unmute(L.lane, ea, es * n, TN_W, ok);
}

__device__ __forceinline__ int z_ud(Lane &L) {
  set_fault(L, WTFGPU_VEC_UD, 0, 0);
  return X_FAULT;
}

__device__ __noinline__ int evex_exec(const Dev &P, Lane &L, const UOp &u, u64 nrip, u64 &next) {
  next = nrip;
  const u32 x = u.opreg, c = u.sub, pp = u.bsz, map = vex_map(x), w = (x >> 2) & 1;
  const u32 ll = evex_ll(x), z = (x >> 21) & 1, b = (x >> 22) & 1, aaa = (x >> 23) & 7, vvvv = evex_vvvv(x);
  const bool mem = u.is_mem;
  const EForm f = evex_form(map, c, pp, w);
  wtfgpu_regs_t &F = P.full[L.lane];
  // ---- #UD: a prefix before EVEX, the AVX-512 state off, encodings the form forbids
  bool ud = ((x >> 16) & 1) || f.kind == EZ_NONE || ll == 3;
  if (!((P.sys[L.lane].cr4 >> 18) & 1) || (F.xcr0 & 0xe6) != 0xe6) ud = true;
  const bool two = f.kind == EZ_MOV || f.kind == EZ_BCAST || f.kind == EZ_BCASTR;
  if (two && vvvv != 0) ud = true;
  if (b && (!mem || !f.bcastok)) ud = true;          // no rounding control in these forms
  if (z && (f.kdest || (f.store && mem) || aaa == 0)) ud = true;  // a k or memory destination merges only; z needs a mask
  if (f.nt && (!mem || aaa != 0)) ud = true;                        // non-temporal moves: memory, no mask
  if (f.kind == EZ_BCASTR && mem) ud = true;
  if (ud) return z_ud(L);
  if (L.cr0 & 8) {
    set_fault(L, 7, 0, 0);  // #NM
    return X_FAULT;
  }
  const u32 vl = 16u << ll, es = f.es, n = vl / es;
  const u64 all = kmask_bits(n), sel = aaa ? (F.k[aaa] & all) : all;
  const u64 ea = mem ? sse_ea(P, L, u, nrip) : 0;
  if (mem && f.aligned && sel && (ea & (vl - 1))) {  // no #GP when every element is masked off
    set_fault(L, WTFGPU_VEC_GP, 0, 0);
    return X_FAULT;
  }
  const u32 dst = u.reg & 31;
  // ---- stores
  if (f.kind == EZ_MOV && f.store && mem) {
    const Z512 s = zmm_get(P, L, dst);
    return zstore(L, ea, es, n, sel, aaa != 0, s) ? X_OK : X_FAULT;
  }
  // ---- the r/m source (a broadcast element, the selected elements, or a register)
  Z512 bsrc;
  if (f.kind == EZ_BCASTR) {
    for (u32 i = 0; i < 8; i++) bsrc.q[i] = 0;
    zset(bsrc, 0, es, R(L, u.rm & 15) & szmask(es));
  } else if (mem) {
    const bool one = b || f.kind == EZ_BCAST;
    // the elements the result needs: a k destination's and a merge's
    // masked-off ones are not read (fault suppression)
    if (!zload(L, ea, one ? es : es, one ? 1 : n, one ? (sel ? 1ull : 0ull) : sel, bsrc)) return X_FAULT;
    if (b) {
      const u64 e0 = zel(bsrc, 0, es);
      for (u32 i = 0; i < n; i++) zset(bsrc, i, es, e0);
    }
  } else {
    bsrc = zmm_get(P, L, (f.store ? dst : u.rm) & 31);
  }
  const Z512 a = zmm_get(P, L, vvvv);
  const Z512 old = zmm_get(P, L, (f.store && !mem) ? (u.rm & 31) : dst);
  const u32 imm = (u32)u.imm & 0xff;
  if (f.kdest) {  // compares and tests: a mask of n bits
    u64 k = 0;
    for (u32 i = 0; i < n; i++) {
      const u64 p = zel(a, i, es), q = zel(bsrc, i, es);
      bool t;
      switch (f.kind) {
        case EZ_CMPEQ: t = p == q; break;
        case EZ_CMPGT: t = (i64)sext(p, es) > (i64)sext(q, es); break;
        case EZ_TESTM: t = ((p & q) != 0) != (f.sub != 0); break;
        default: {  // EZ_CMP: imm[2:0] 0 eq 1 lt 2 le 3 false 4 neq 5 nlt 6 nle 7 true
          const bool lt = f.sub ? (i64)sext(p, es) < (i64)sext(q, es) : p < q;
          const bool eq = p == q;
          const u32 pr = imm & 7;
          t = pr == 0 ? eq : pr == 1 ? lt : pr == 2 ? (lt || eq) : pr == 3 ? false : pr == 4 ? !eq
              : pr == 5 ? !lt : pr == 6 ? !(lt || eq) : true;
        }
      }
      k |= (u64)t << i;
    }
    F.k[u.reg & 7] = k & sel;
    return X_OK;
  }
  Z512 r = old;
  for (u32 i = 0; i < n; i++) {
    if (!((sel >> i) & 1)) {
      if (z) zset(r, i, es, 0);
      continue;
    }
    const u64 p = zel(a, i, es), q = zel(bsrc, i, es);
    u64 v;
    switch (f.kind) {
      case EZ_MOV: v = q; break;
      case EZ_LOGIC: v = f.sub == 0 ? (p & q) : f.sub == 1 ? (~p & q) : f.sub == 2 ? (p | q) : (p ^ q); break;
      case EZ_ADD: v = p + q; break;
      case EZ_SUB: v = p - q; break;
      case EZ_MINU: v = p < q ? p : q; break;
      case EZ_MAXU: v = p > q ? p : q; break;
      case EZ_TERN: {  // bit j of the result: imm8[(dst << 2) | (src1 << 1) | src2] of bit j
        const u64 d = zel(old, i, es);
        v = 0;
        for (u32 t = 0; t < 8; t++) {
          if (!((imm >> t) & 1)) continue;
          v |= ((t & 4) ? d : ~d) & ((t & 2) ? p : ~p) & ((t & 1) ? q : ~q);
        }
        break;
      }
      default: v = zel(bsrc, 0, es); break;  // broadcasts
    }
    zset(r, i, es, v & szmask(es));
  }
  zmm_put(P, L, (f.store && !mem) ? (u.rm & 31) : dst, r, vl);
  return X_OK;
}

// The VEX-encoded opmask instructions.
__device__ __noinline__ int kop_exec(const Dev &P, Lane &L, const UOp &u, u64 nrip, u64 &next) {
  next = nrip;
  const u32 x = u.opreg, c = u.sub, pp = u.bsz, map = vex_map(x), w = (x >> 2) & 1, l = (x >> 1) & 1;
  const u32 vvvv = (x >> 4) & 15, bits = kop_bits(map, c, pp, w);
  wtfgpu_regs_t &F = P.full[L.lane];
  const bool mem = u.is_mem;
  // VEX.L: 1 for the two-source ops (logic, kadd, kunpck), else 0; vvvv: only they name a register
  const bool two_src = map == 1 && ((c >= 0x41 && c <= 0x47 && c != 0x44) || c == 0x4a || c == 0x4b);
  bool ud = ((x >> 16) & 1) || !bits || l != (two_src ? 1u : 0u) || (!two_src && vvvv != 0);
  if (!((P.sys[L.lane].cr4 >> 18) & 1) || (F.xcr0 & 0xe6) != 0xe6) ud = true;
  if (mem && !(map == 1 && (c == 0x90 || c == 0x91))) ud = true;  // only kmov has memory forms
  if (!mem && map == 1 && c == 0x91) ud = true;
  if (ud) return z_ud(L);
  const u64 mk = kmask_bits(bits);
  const u32 kr = u.reg & 7, km = u.rm & 7;
  if (map == 3) {  // kshiftr / kshiftl
    const u32 cnt = (u32)u.imm & 0xff;
    const u64 s = F.k[km] & mk;
    F.k[kr] = cnt >= bits ? 0 : (((c & 2) ? (s << cnt) : (s >> cnt)) & mk);
    return X_OK;
  }
  switch (c) {
    case 0x90:
      if (mem) {
        u64 v;
        if (!vread(L, sse_ea(P, L, u, nrip), bits / 8, v)) return X_FAULT;
        F.k[kr] = v & mk;
      } else {
        F.k[kr] = F.k[km] & mk;
      }
      return X_OK;
    case 0x91: return vwrite(L, sse_ea(P, L, u, nrip), bits / 8, F.k[kr] & mk) ? X_OK : X_FAULT;
    case 0x92: F.k[kr] = R(L, u.rm & 15) & mk; return X_OK;
    case 0x93: RS(L, u.reg & 15, F.k[km] & mk); return X_OK;  // a 32-bit destination zero-extended
    case 0x98:
    case 0x99: {
      const u64 p = F.k[kr] & mk, q = F.k[km] & mk;
      const bool zf = c == 0x98 ? (p | q) == 0 : (p & q) == 0;
      const bool cf = c == 0x98 ? (p | q) == mk : (~p & q & mk) == 0;
      L.rflags = (L.rflags & ~F_STATUS) | (zf ? F_ZF : 0) | (cf ? F_CF : 0);
      return X_OK;
    }
    case 0x44: F.k[kr] = ~F.k[km] & mk; return X_OK;
    case 0x4b: {  // kunpck: the first source's low half above the second source's low half
      const u32 h = bits / 2;
      const u64 hm = kmask_bits(h);
      F.k[kr] = ((F.k[vvvv & 7] & hm) << h) | (F.k[km] & hm);
      return X_OK;
    }
    default: {
      const u64 p = F.k[vvvv & 7] & mk, q = F.k[km] & mk;
      const u64 v = c == 0x41 ? (p & q) : c == 0x42 ? (~p & q) : c == 0x45 ? (p | q) : c == 0x46 ? ~(p ^ q)
                  : c == 0x4a ? p + q : (p ^ q);  // 4a: kadd
      F.k[kr] = v & mk;
      return X_OK;
    }
  }
}

}  // namespace wtfgpu_dev
