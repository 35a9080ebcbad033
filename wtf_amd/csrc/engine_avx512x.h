// engine_avx512x.h — the AVX-512 integer forms of DESIGN.md U49: element-wise
// arithmetic, shifts and rotates, the in-lane shuffles, the cross-lane
// permutes and the widening loads (the table is evex_form's, engine_avx512.h;
// kinds from EZ_X on), and the block, mask and GPR moves (kinds from EZ_Y on:
// evexm_exec, at the end). evexx_exec runs them on the generic step, beside
// evex_exec and with its rules: #UD, #NM, then the memory access; a masked-off
// element of a memory source is not read unless the form has no fault
// suppression (XF_NF: the shuffles, permutes and xmm-count shifts read their
// whole operand); nothing is written before every access succeeded.
//
// Scratch: the frame holds two Z512 — the r/m source and the result. The
// other sources (vvvv, the old destination, vpermi2's index, vpermt2's first
// table) are fetched an element at a time from the lane's state in memory
// (P.full[lane]) by computed address; the result is assembled in registers
// and written last, so a destination that aliases a source needs no copy.
#pragma once

namespace wtfgpu_dev {

// qword qi of zmm r, and element i (w bytes) of it, straight from the state
__device__ __forceinline__ u64 zq(const wtfgpu_regs_t &F, u32 r, u32 qi) {
  if (r >= 16) return F.zmm_hi[r - 16][qi];
  return qi < 2 ? F.xmm[r][qi] : qi < 4 ? F.ymmh[r][qi - 2] : F.zmmh[r][qi - 4];
}
__device__ __forceinline__ u64 zre(const wtfgpu_regs_t &F, u32 r, u32 i, u32 w) {
  const u32 bit = i * w * 8;
  return (zq(F, r, bit >> 6) >> (bit & 63)) & szmask(w);
}

// A shift or rotate of one element; cnt is the whole count (an imm8, the xmm
// count's low qword, or the count element): past the width a logical shift
// gives 0 and an arithmetic one the sign, a rotate takes it modulo the width.
__device__ __forceinline__ u64 xshift(u32 op, u64 v, u64 cnt, u32 es) {
  const u32 bits = es * 8;
  const u32 k = (u32)cnt & (bits - 1);
  switch (op) {
    case XS_SRL: return cnt >= bits ? 0 : v >> cnt;
    case XS_SLL: return cnt >= bits ? 0 : v << cnt;
    case XS_SRA: return (u64)((i64)sext(v, es) >> (cnt >= bits ? 63 : cnt));
    case XS_ROR: return k ? (v >> k) | (v << (bits - k)) : v;
    default: return k ? (v << k) | (v >> (bits - k)) : v;  // XS_ROL
  }
}

__device__ __forceinline__ u64 xbin(u32 op, u64 p, u64 q, u32 es) {
  const i64 sp = (i64)sext(p, es), sq = (i64)sext(q, es);
  switch (op) {
    case XB_MINS: return sp < sq ? p : q;
    case XB_MAXS: return sp > sq ? p : q;
    case XB_MINU: return p < q ? p : q;
    case XB_MAXU: return p > q ? p : q;
    case XB_ADDS: return sat_s(sp + sq, es);  // bytes and words only
    case XB_ADDUS: return sat_u((i64)(p + q), es);
    case XB_SUBS: return sat_s(sp - sq, es);
    case XB_SUBUS: return p > q ? p - q : 0;
    case XB_AVG: return (p + q + 1) >> 1;
    case XB_MULL: return p * q;
    case XB_MULH: return (u64)((sp * sq) >> 16);  // words
    case XB_MULHU: return (p * q) >> 16;
    case XB_MULUDQ: return (p & 0xffffffffull) * (q & 0xffffffffull);
    case XB_MULDQ: return (u64)((i64)(i32)(u32)p * (i64)(i32)(u32)q);
    case XB_SLLV: return xshift(XS_SLL, p, q, es);
    case XB_SRLV: return xshift(XS_SRL, p, q, es);
    case XB_SRAV: return xshift(XS_SRA, p, q, es);
    case XB_ROLV: return xshift(XS_ROL, p, q, es);
    default: return xshift(XS_ROR, p, q, es);  // XB_RORV
  }
}

__device__ __noinline__ int evexx_exec(const Dev &P, Lane &L, const UOp &u, u64 nrip, u64 &next) {
  next = nrip;
  const u32 x = u.opreg, c = u.sub, pp = u.bsz, map = vex_map(x), w = (x >> 2) & 1;
  const u32 ll = evex_ll(x), z = (x >> 21) & 1, b = (x >> 22) & 1, aaa = (x >> 23) & 7, vvvv = evex_vvvv(x);
  const bool mem = u.is_mem;
  const EForm f = evex_form(map, c, pp, w, u.reg & 7);
  wtfgpu_regs_t &F = P.full[L.lane];
  const bool nf = (f.fl & XF_NF) != 0;
  // ---- #UD: a prefix before EVEX, the AVX-512 state off, encodings the form forbids
  bool ud = ((x >> 16) & 1) || f.kind < EZ_X || ll == 3;
  if (!((P.sys[L.lane].cr4 >> 18) & 1) || (F.xcr0 & 0xe6) != 0xe6) ud = true;
  if ((f.fl & XF_TWO) && vvvv != 0) ud = true;
  if (b && (!mem || !f.bcastok)) ud = true;  // no rounding control in these forms
  if (z && aaa == 0) ud = true;
  if ((f.fl & XF_NOMASK) && aaa != 0) ud = true;
  if ((f.fl & XF_NO128) && ll == 0) ud = true;
  if (ud) return z_ud(L);
  if (L.cr0 & 8) {
    set_fault(L, 7, 0, 0);  // #NM
    return X_FAULT;
  }
  const u32 vl = 16u << ll, es = f.es, ses = f.ses, n = vl / es;
  const u64 all = kmask_bits(n), sel = aaa ? (F.k[aaa] & all) : all;
  const u32 dst = (f.fl & XF_VDST) ? vvvv : (u.reg & 31);
  // ---- the r/m source: a broadcast element, the operand's selected elements, or a register
  Z512 bs;
  if (mem) {
    const u64 ea = sse_ea(P, L, u, nrip);
    if (b) {
      if (!zload(L, ea, ses, 1, (sel || nf) ? 1ull : 0ull, bs)) return X_FAULT;
      const u64 e0 = zel(bs, 0, ses);
      for (u32 i = 0; i < vl / ses; i++) zset(bs, i, ses, e0);
    } else if (f.mc == MC_M128) {
      if (!zload(L, ea, 8, 2, 3, bs)) return X_FAULT;
    } else if (f.kind == EZ_PMOVX) {
      if (!zload(L, ea, ses, n, sel, bs)) return X_FAULT;
    } else if (nf) {
      if (!zload(L, ea, 8, vl / 8, kmask_bits(vl / 8), bs)) return X_FAULT;
    } else {
      if (!zload(L, ea, es, n, sel, bs)) return X_FAULT;
    }
  } else {
    bs = zmm_get(P, L, u.rm & 31);
  }
  const u32 imm = (u32)u.imm & 0xff;
  const u64 cntx = bs.q[0];  // EZ_SHX: the count
  Z512 r;
  for (u32 i = 0; i < 8; i++) r.q[i] = zq(F, dst, i);
  for (u32 i = 0; i < n; i++) {
    if (!((sel >> i) & 1)) {
      if (z) zset(r, i, es, 0);
      continue;
    }
    u64 v = 0;
    switch (f.kind) {
      case EZ_BIN: v = xbin(f.sub, zre(F, vvvv, i, es), zel(bs, i, es), es); break;
      case EZ_UN: {  // vpabs
        const i64 s = (i64)sext(zel(bs, i, es), es);
        v = s < 0 ? 0 - (u64)s : (u64)s;  // unsigned: the minimum value maps to itself
        break;
      }
      case EZ_SHI: v = xshift(f.sub, zel(bs, i, es), imm, es); break;
      case EZ_SHX: v = xshift(f.sub, zre(F, vvvv, i, es), cntx, es); break;
      case EZ_BSH: {  // vpsrldq (sub 0) / vpslldq (1): bytes within the 128-bit lane
        const u32 j = i & 15, t = f.sub ? j - imm : j + imm;
        v = (imm < 16 && t < 16) ? zel(bs, (i & ~15u) + t, 1) : 0;
        break;
      }
      case EZ_PSHUFB: {
        const u32 s = (u32)zel(bs, i, 1);
        v = (s & 0x80) ? 0 : zre(F, vvvv, (i & ~15u) | (s & 15), 1);
        break;
      }
      case EZ_PSHUFD: v = zel(bs, (i & ~3u) | ((imm >> (2 * (i & 3))) & 3), 4); break;
      case EZ_PSHUFW: {  // vpshuflw (sub 0): words 0-3 of each lane; vpshufhw (1): words 4-7
        const u32 j = i & 7, hi = f.sub ? 4u : 0u;
        v = (j >= hi && j < hi + 4) ? zel(bs, (i & ~7u) + hi + ((imm >> (2 * (j - hi))) & 3), 2) : zel(bs, i, 2);
        break;
      }
      case EZ_UNPCK: {  // sub: the lane's high half
        const u32 m = 16 / es, j = i % m, s = (i - j) + (f.sub ? m / 2 : 0) + j / 2;
        v = (j & 1) ? zel(bs, s, es) : zre(F, vvvv, s, es);
        break;
      }
      case EZ_PACK: {  // per lane: the first source's elements, then the second's; sub: unsigned saturation
        const u32 m = 16 / es, j = i % m, s = (i / m) * (m / 2) + j % (m / 2);
        const i64 e = (i64)sext(j < m / 2 ? zre(F, vvvv, s, ses) : zel(bs, s, ses), ses);
        v = f.sub ? sat_u(e, es) : sat_s(e, es);
        break;
      }
      case EZ_ALIGNR: {  // per lane: (first : second) >> imm bytes
        const u32 t = (i & 15) + imm, lb = i & ~15u;
        v = t < 16 ? zel(bs, lb + t, 1) : t < 32 ? zre(F, vvvv, lb + t - 16, 1) : 0;
        break;
      }
      case EZ_PERM: v = zel(bs, (u32)zre(F, vvvv, i, es) & (n - 1), es); break;
      case EZ_PERMQI: v = zel(bs, (i & ~3u) | ((imm >> (2 * (i & 3))) & 3), 8); break;
      case EZ_PERMI2: {  // the destination holds the indices
        const u32 s = (u32)zre(F, dst, i, es);
        v = (s & n) ? zel(bs, s & (n - 1), es) : zre(F, vvvv, s & (n - 1), es);
        break;
      }
      case EZ_PERMT2: {  // the destination is the first table
        const u32 s = (u32)zre(F, vvvv, i, es);
        v = (s & n) ? zel(bs, s & (n - 1), es) : zre(F, dst, s & (n - 1), es);
        break;
      }
      case EZ_VALIGN: {  // (first : second) >> imm elements
        const u32 t = i + (imm & (n - 1));
        v = t < n ? zel(bs, t, es) : zre(F, vvvv, t - n, es);
        break;
      }
      case EZ_SHUFI: {  // 128-bit blocks: the low half of the result from the first source, the high from the second
        const u32 nb = vl / 16, epb = 16 / es, blk = i / epb, bits = nb == 4 ? 2u : 1u;
        const u32 s = ((imm >> (blk * bits)) & (nb - 1)) * epb + i % epb;
        v = blk < nb / 2 ? zre(F, vvvv, s, es) : zel(bs, s, es);
        break;
      }
      default: {  // EZ_PMOVX: sub signed
        const u64 e = zel(bs, i, ses);
        v = f.sub ? sext(e, ses) : e;
        break;
      }
    }
    zset(r, i, es, v & szmask(es));
  }
  zmm_put(P, L, dst, r, vl);
  return X_OK;
}

// The block, mask and GPR moves (kinds from EZ_Y on): vinserti / vextracti /
// vbroadcasti 32x4, 64x2, 32x8, 64x4 (and 32x2), vpmovm2* / vpmov*2m, vmovd /
// vmovq. None has a broadcast form; f.ses is the block's bytes.
__device__ __noinline__ int evexm_exec(const Dev &P, Lane &L, const UOp &u, u64 nrip, u64 &next) {
  next = nrip;
  const u32 x = u.opreg, c = u.sub, pp = u.bsz, map = vex_map(x), w = (x >> 2) & 1;
  const u32 ll = evex_ll(x), z = (x >> 21) & 1, b = (x >> 22) & 1, aaa = (x >> 23) & 7, vvvv = evex_vvvv(x);
  const bool mem = u.is_mem;
  const EForm f = evex_form(map, c, pp, w, u.reg & 7);
  wtfgpu_regs_t &F = P.full[L.lane];
  bool ud = ((x >> 16) & 1) || f.kind < EZ_Y || ll == 3 || b;
  if (!((P.sys[L.lane].cr4 >> 18) & 1) || (F.xcr0 & 0xe6) != 0xe6) ud = true;
  if ((f.fl & XF_TWO) && vvvv != 0) ud = true;
  if (z && (aaa == 0 || (f.kind == EZ_EXT && mem))) ud = true;  // a memory destination merges only
  if ((f.fl & XF_NOMASK) && aaa != 0) ud = true;
  if (((f.fl & XF_NO128) && ll == 0) || ((f.fl & XF_ONLY512) && ll != 2) || ((f.fl & XF_ONLY128) && ll != 0)) ud = true;
  if (((f.fl & XF_MEMONLY) && !mem) || ((f.fl & XF_REGONLY) && mem)) ud = true;
  if (ud) return z_ud(L);
  if (L.cr0 & 8) {
    set_fault(L, 7, 0, 0);  // #NM
    return X_FAULT;
  }
  const u32 vl = 16u << ll, es = f.es, blk = f.ses;
  const u64 ea = mem ? sse_ea(P, L, u, nrip) : 0;
  const u32 reg = u.reg & 31, rm = u.rm & 31;
  const u32 imm = (u32)u.imm & 0xff;
  Z512 r;
  switch (f.kind) {
    case EZ_GMOV: {
      u64 v = 0;
      if (f.sub == 0 || f.sub == 2) {  // to xmm, the rest of the register zeroed
        if (mem) {
          if (!vread(L, ea, es, v)) return X_FAULT;
        } else {
          v = f.sub == 0 ? (R(L, u.rm & 15) & szmask(es)) : zq(F, rm, 0);
        }
        for (u32 i = 0; i < 8; i++) r.q[i] = 0;
        r.q[0] = v;
        zmm_put(P, L, reg, r, 16);
        return X_OK;
      }
      v = zq(F, reg, 0) & szmask(es);
      if (mem) return vwrite(L, ea, es, v) ? X_OK : X_FAULT;
      if (f.sub == 1) {
        RS(L, u.rm & 15, v);  // a 32-bit destination zero-extended
      } else {
        for (u32 i = 0; i < 8; i++) r.q[i] = 0;
        r.q[0] = v;
        zmm_put(P, L, rm, r, 16);
      }
      return X_OK;
    }
    case EZ_M2V: {
      const u32 n = vl / es;
      const u64 k = F.k[u.rm & 7];
      for (u32 i = 0; i < 8; i++) r.q[i] = 0;
      for (u32 i = 0; i < n; i++) zset(r, i, es, ((k >> i) & 1) ? szmask(es) : 0);
      zmm_put(P, L, reg, r, vl);
      return X_OK;
    }
    case EZ_V2M: {
      const u32 n = vl / es;
      u64 k = 0;
      for (u32 i = 0; i < n; i++) k |= ((zre(F, rm, i, es) >> (es * 8 - 1)) & 1) << i;
      F.k[u.reg & 7] = k;
      return X_OK;
    }
    case EZ_EXT: {  // block imm of the source (reg) to the r/m register or memory, masked by element
      const u32 n = blk / es, pos = imm & (vl / blk - 1);
      const u64 sel = aaa ? (F.k[aaa] & kmask_bits(n)) : kmask_bits(n);
      for (u32 i = 0; i < 8; i++) r.q[i] = mem ? 0 : zq(F, rm, i);
      for (u32 i = 0; i < n; i++) {
        if ((sel >> i) & 1) zset(r, i, es, zre(F, reg, pos * n + i, es));
        else if (z) zset(r, i, es, 0);
      }
      if (mem) {  // no fault suppression: the whole block is probed whatever the mask, then the selected elements written
        if (!span_ok(L, ea, blk, ACC_WPROBE)) return X_FAULT;
        return zstore(L, ea, es, n, sel, false, r) ? X_OK : X_FAULT;
      }
      zmm_put(P, L, rm, r, blk);
      return X_OK;
    }
    default: {  // EZ_INS, EZ_BCB: a block from r/m into the result, masked by element
      const u32 n = vl / es, m = blk / es;
      const u64 sel = aaa ? (F.k[aaa] & kmask_bits(n)) : kmask_bits(n);
      Z512 bs;
      if (mem) {
        // vinserti reads its block whatever the mask; a broadcast reads the block's elements some
        // selected element takes
        u64 need = kmask_bits(m);
        if (f.kind == EZ_BCB) {
          need = 0;
          for (u32 i = 0; i < n; i++) need |= ((sel >> i) & 1) << (i % m);
        }
        if (!zload(L, ea, es, m, need, bs)) return X_FAULT;
      } else {
        bs = zmm_get(P, L, rm);
      }
      const u32 pos = imm & (vl / blk - 1);
      for (u32 i = 0; i < 8; i++) r.q[i] = zq(F, reg, i);
      for (u32 i = 0; i < n; i++) {
        if (!((sel >> i) & 1)) {
          if (z) zset(r, i, es, 0);
          continue;
        }
        const u64 v = (f.kind == EZ_BCB || i / m == pos) ? zel(bs, i % m, es) : zre(F, vvvv, i, es);
        zset(r, i, es, v);
      }
      zmm_put(P, L, reg, r, vl);
      return X_OK;
    }
  }
}

}  // namespace wtfgpu_dev
