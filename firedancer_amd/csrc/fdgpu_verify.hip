/* fdgpu_verify.hip -- MI355X (gfx950) kernels of the batched Ed25519 verify.
   One signature per lane, 256-thread workgroups; integer / bignum work only
   (no MFMA).  Per batch, on one stream:

   fdgpu_verify_hs_kernel  everything: S < L,
       k = SHA-512(R||A||M) mod L, decode A and R (decode2's rules and code
       order) with their small-order tests and the per-lane tables
       {O, -A, .., -8A}, {O, -R, .., -8R}; the lattice split of k into two
       ~128-bit scalars u = v k (mod 8L) (fdgpu_lattice.h); [w]B (w = v S
       mod L) by the fixed-base comb; [u](+-A) + [v](+-R) on one shared,
       divergence-free signed radix-16 chain with the table entries staged
       through LDS by LDS-DMA; the projective check against -[w]B.
   fdgpu_full_kernel       the rare lanes whose split failed: the full-length
       [S]B + [k](-A) chain, compared with the decoded R.
   fdgpu_key_dedup_kernel, fdgpu_key_table_kernel  (FDGPU_FLAG_KCACHE) one A
       decode + table per distinct public key, read in place by
       fdgpu_verify_hs_kernel<true> and the fallback kernel.
   fdgpu_combine_kernel    per transaction, batch_single_msg first-error
       semantics (fd_ed25519_user.c:232-310), plus a ballot-compacted
       accept bitmap.
   The other kernels of the library live in units of their own: the comb
   tables' build (fdgpu_bcomb.hip), the GPU-side ingest (fdgpu_ingest.hip),
   the per-stage diagnostics (fdgpu_test_kernels.hip), raw shreds
   (fdgpu_shred.hip). */
#include <hip/hip_runtime.h>

#include "fdgpu_atab.h"
#include "fdgpu_bcomb.h"
#include "fdgpu_ge.h"
#include "fdgpu_hram.h"
#include "fdgpu_internal.h"
#include "fdgpu_lattice.h"
#include "fdgpu_sc.h"
#include "fdgpu_sha512.h"
#include "fdgpu_stamps.h"

using namespace fdgpu;

namespace {

/* ---- per-lane tables in the global workspace ----
   lane i's 16 stored entries (1..8 of its -A table, then 1..8 of its -R
   table) are the 2 KiB at ws + i * FDGPU_WS_TAB_WORDS, each a packed entry
   of one 128-B line (fdgpu_atab.h: atab_store / atab_load and the LDS path
   convert, every other reader sees canonical-order limbs); its park entry
   and [w]B are plain words in the aux region behind the tables
   (fdgpu_internal.h). */

/* virtual bases of a lane's -A and -R tables: stored entry 1 sits at the
   table's first workspace entry */
FDG_DEV uint32_t *tab_a(uint32_t *wsl) { return wsl - FDGPU_PTAB_WORDS; }
FDG_DEV const uint32_t *tab_a(const uint32_t *wsl) { return wsl - FDGPU_PTAB_WORDS; }
FDG_DEV uint32_t *tab_r(uint32_t *wsl) { return wsl + (FDGPU_WS_RTAB - 1u) * FDGPU_PTAB_WORDS; }

/* [w]B (or [S]B) of a lane: an unpacked cached entry in canonical order at
   the lane's aux words (written once and read once per signature) */
FDG_DEV void sb_store(uint32_t *aux, const ge_cached &c) {
  uint4 *p = (uint4 *)(aux + FDGPU_AUX_SB);
  uint32_t w[40];
#pragma unroll
  for (int i = 0; i < 10; i++) { w[i] = c.YpX.v[i]; w[10 + i] = c.YmX.v[i]; w[20 + i] = c.Z2.v[i]; w[30 + i] = c.T2d.v[i]; }
#pragma unroll
  for (int q = 0; q < 10; q++) p[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}
FDG_DEV void sb_load(uint32_t (&q)[40], const uint32_t *aux) {
  const uint4 *ent = (const uint4 *)(aux + FDGPU_AUX_SB);
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint4 v = ent[i];
    q[4 * i] = v.x; q[4 * i + 1] = v.y; q[4 * i + 2] = v.z; q[4 * i + 3] = v.w;
  }
}
FDG_DEV int sext4(uint32_t x) { return ((int)(x << 28)) >> 28; }

#define KD_WORDS 8        /* 64 signed radix-16 digits of k, one per nibble */

/* shift a 256-bit little-endian word vector left by 4 bits */
FDG_DEV void shl4(uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 7; i > 0; i--) w[i] = (w[i] << 4) | (w[i - 1] >> 28);
  w[0] <<= 4;
}

/* R' = [k](-A) + [S]B with [S]B precomputed by the
   comb in pass 1 and parked (cached form) in the lane's aux words.  The chain
   only serves k: 64 windows of 4 doublings + one A-table addition; the last
   window's sum is converted to p3 and the parked [S]B added. */
FDG_DEV void dsm_k(ge_p2 &acc2, uint32_t (&kd)[KD_WORDS], const uint32_t *aux, const uint32_t *ta) {
  /* ta: the -A table, own workspace or the key cache's */
  ge_p3 acc3;
  ge_p1p1 t;
  uint32_t q[40];
  /* the top window would double the identity four times and then add its
     entry: start from the entry itself (Horner's first step) */
  {
    const int e = sext4(kd[7] >> 28);
    shl4(kd);
    atab_load(q, ta, e);
    ge_cached_regs_to_p2(acc2, q, e < 0);
  }
#pragma unroll 1
  for (int j = 62; j >= 0; j--) {
    const int e = sext4(kd[7] >> 28);
    shl4(kd);
    atab_load(q, ta, e);
#pragma unroll 1
    for (int r = 0; r < 4; r++) {
      ge_dbl(t, acc2);
      ge_p1p1_to_p2(acc2, t);
    }
    acc3.X = acc2.X; acc3.Y = acc2.Y; acc3.Z = acc2.Z; fe_mul(acc3.T, t.X, t.Y);
    ge_add_cached_regs(t, acc3, q, e < 0);
    if (j == 0) break;
    ge_p1p1_to_p2(acc2, t);
  }
  /* + [S]B (parked cached form) */
  ge_p1p1_to_p3(acc3, t);
  uint32_t qs[40];
  sb_load(qs, aux);
  ge_add_cached_regs(t, acc3, qs, false);
  ge_p1p1_to_p2(acc2, t);
}

/* [S]B by the fixed-base comb: S (< L, or 0 for rejected lanes) in signed
   radix 2^W; one mixed addition per digit from table i; each entry (one
   128-B line, random across the 67-MB table) is loaded one digit ahead of
   its use so the load latency hides behind the previous addition.  [lo, hi)
   sums only the digits of tables lo..hi-1 (the two-lane kernel splits the
   comb over a pair: 2 + 2 x 7 additions instead of 15 per lane). */
FDG_DEV void comb_sb(ge_p3 &acc, const uint32_t (&S)[8], const uint32_t *__restrict__ btab, uint32_t lo = 0,
                     uint32_t hi = BC_NDIG) {
  constexpr int NW = COMB_WORDS(BC_W, BC_NDIG), SLOT = COMB_SLOT(BC_W);
  uint32_t dg[NW];
  sc_recode_comb<(int)BC_W, (int)BC_NDIG>(dg, S);
  auto next_digit = [&dg]() {
    const int d = SLOT == 16 ? (int)(int16_t)(dg[0] & 0xffffu) : (int)dg[0];
#pragma unroll
    for (int i = 0; i < NW - 1; i++) dg[i] = SLOT == 16 ? (dg[i] >> 16) | (dg[i + 1] << 16) : dg[i + 1];
    dg[NW - 1] = SLOT == 16 ? dg[NW - 1] >> 16 : 0u;
    return d;
  };
  auto load_entry = [btab](uint32_t (&q)[32], uint32_t ti, int d) {
    const uint4 *ent = (const uint4 *)(btab + ((size_t)ti * BC_ENT + (uint32_t)(d < 0 ? -d : d)) * FDGPU_BCOMB_STRIDE);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint4 v = ent[i];
      q[4 * i] = v.x; q[4 * i + 1] = v.y; q[4 * i + 2] = v.z; q[4 * i + 3] = v.w;
    }
  };
  uint32_t qa[32], qb[32];
#pragma unroll 1
  for (uint32_t i = 0; i < lo; i++) (void)next_digit();
  int d = next_digit();
  load_entry(qa, lo, d);
  /* the first digit's entry is the starting point (no addition to O) */
  {
    const int dn = next_digit();
    load_entry(qb, lo + 1, dn);
    ge_niels_regs_to_p3(acc, qa, d < 0);
#pragma unroll
    for (int w = 0; w < 32; w++) qa[w] = qb[w];
    d = dn;
  }
  ge_p1p1 t;
#pragma unroll 1
  for (uint32_t i = lo + 1; i < hi; i++) {
    const int dn = next_digit();
    if (i + 1 < hi) load_entry(qb, i + 1, dn);
    ge_add_niels_regs(t, acc, qa, d < 0);
    ge_p1p1_to_p3(acc, t);
#pragma unroll
    for (int w = 0; w < 32; w++) qa[w] = qb[w];
    d = dn;
  }
}

/* Build this lane's table {-A, -2A, ..., -8A} (cached form; O is the
   shared g_tab_ident) in the workspace.  Even multiples by doubling the stored half (4S + 4M) instead
   of adding -A (8M): 3 = 2 + 1, 4 = 2*2, 5 = 4 + 1, 6 = 2*3, 7 = 6 + 1,
   8 = 2*4. */
FDG_DEV void atab_build(uint32_t *wsl, const ge_p3 &An) {   /* wsl: the table's virtual base (tab_a / tab_r) */
  ge_cached c;
  ge_p3_to_cached(c, An); atab_store(wsl, 1, c);
  ge_p1p1 t; ge_p2 a2; ge_p3 P;
  ge_p3_to_p2(a2, An); ge_dbl(t, a2); ge_p1p1_to_p3(P, t);          /* 2(-A) */
  ge_p3_to_cached(c, P); atab_store(wsl, 2, c);
  const uint32_t *ent1 = wsl + 1u * FDGPU_PTAB_WORDS;
  auto ld1 = [ent1](int cc, int w) { return atab_limb(ent1, cc, w); };
#pragma unroll 1
  for (uint32_t e = 3; e < FDGPU_ATAB_ENTRIES; e++) {
    if (e & 1u) {
      ge_add_cached_ld(t, P, ld1, false);
    } else {
      uint32_t q[40];
      atab_load(q, wsl, (int)(e >> 1));
      ge_cached_regs_to_p2(a2, q, false);
      ge_dbl(t, a2);
    }
    ge_p1p1_to_p3(P, t);
    ge_p3_to_cached(c, P); atab_store(wsl, e, c);
  }
}

/* lane i's 16 table entries (2 KiB, line-aligned) */
FDG_DEV uint32_t *lane_ws(uint32_t *ws, uint32_t i) {
  return ws + (size_t)i * FDGPU_WS_TAB_WORDS;
}
/* lane i's aux words (park entry, [w]B), counted back from the aux region's
   end, which is the fallback queue's first word (fdgpu_ws_layout) */
FDG_DEV uint32_t *lane_aux(uint32_t *queue, uint32_t i) {
  return queue - ((size_t)i + 1u) * FDGPU_WS_AUX_WORDS;
}
FDG_DEV const uint32_t *lane_aux(const uint32_t *queue, uint32_t i) {
  return queue - ((size_t)i + 1u) * FDGPU_WS_AUX_WORDS;
}

/* Output slot of lane i: signatures may be verified in an order grouped by
   SHA-512 block count (perm[i] = the signature's index in the caller's
   order); codes are always written in the caller's order. */
FDG_DEV uint32_t out_idx(const uint32_t *__restrict__ perm, uint32_t i) { return perm ? perm[i] : i; }

/* ---------------- half-size verify ----------------
   fdgpu_lattice.h: with u = v k (mod 8L), v odd and |u|, |v| < 2^159,
   [S]B - [k]A == R  <=>  [w]B - [u]A - [v]R == O  (w = v S mod L), decided
   with ~132 doublings instead of ~252.  Per lane:
     pass 1   S < L, k = SHA-512(R||A||M) mod L, decode A and R (the
              reference's decode2, both codes settled here in the
              reference's order), the tables {O, -A, .., -8A} and
              {O, -R, .., -8R};
     split    (u, v) = hs_split(k);  w = v S mod L;  [w]B by the comb;
     chain    [|u|](+-A table) + [|v|](+-R table) over the wave's longest
              digit string (signed radix 16: 4 doublings + 2 additions per
              window, every lane at the same positions);
     check    chain == -[w]B, projectively (4 products).
   A lane whose split fails (hs_split_t.ok == false) keeps k's digits and
   [S]B and is finished by fdgpu_full_kernel with the full-length chain. */

/* park words (a lane's aux words from FDGPU_AUX_PARK) */
#define HPARK_KD 0        /* 8 words: radix-16 digits of k (full-path lanes) */
#define HPARK_CODE 30     /* pass-1 code */
/* (decoded R is not parked: fdgpu_full_kernel compares with the -R table's
   entry 1, projectively, so a half-size lane never writes this entry) */
static_assert(HPARK_KD + KD_WORDS <= HPARK_CODE && HPARK_CODE < (int)FDGPU_AUX_SB - (int)FDGPU_AUX_PARK &&
              FDGPU_AUX_SB + FDGPU_ATAB_WORDS <= FDGPU_WS_AUX_WORDS && FDGPU_AUX_SB % 4u == 0 && FDGPU_WS_AUX_WORDS % 4u == 0,
              "aux layout");

/* Signed radix-16 digits of a magnitude m < 2^160 (5 limbs): 40 nibbles in
   [-8, 7] (two's complement, digit i at bits 4(i%8) of word i/8); nd = the
   number of digits up to the highest nonzero one (41 if a carry is left). */
FDG_DEV void recode16_160(uint32_t (&out)[5], uint32_t &nd, const uint32_t (&m)[5]) {
  uint32_t carry = 0;
  nd = 0;
#pragma unroll
  for (int w = 0; w < 5; w++) {
    uint32_t o = 0;
#pragma unroll
    for (int n = 0; n < 8; n++) {
      uint32_t e = ((m[w] >> (4 * n)) & 15u) + carry;
      carry = e >= 8u;
      e = (e - (carry << 4)) & 15u;
      o |= e << (4 * n);
      nd = e ? (uint32_t)(8 * w + n + 1) : nd;
    }
    out[w] = o;
  }
  nd = carry ? 41u : nd;
}

FDG_DEV void shl4_5(uint32_t (&w)[5]) {
#pragma unroll
  for (int i = 4; i > 0; i--) w[i] = (w[i] << 4) | (w[i - 1] >> 28);
  w[0] <<= 4;
}

/* w = v S mod L for |v| < 2^160 (5 limbs), S < L (8 limbs); negated mod L
   when v < 0 */
FDG_DEV void hs_wscalar(uint32_t (&w)[8], const uint32_t (&v)[5], bool v_neg, const uint32_t (&S)[8]) {
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 16; i++) x[i] = 0;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t t = (uint64_t)v[i] * S[j] + x[i + j] + c;
      x[i + j] = (uint32_t)t;
      c = t >> 32;
    }
    x[i + 8] = (uint32_t)c;
  }
  uint32_t r[8];
  sc_reduce512(r, x);
  constexpr uint32_t L[8] = FDGPU_SC_L;
  uint32_t nz = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) nz |= r[i];
  const bool flip = v_neg && nz != 0;
  uint32_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {                 /* L - r */
    const uint64_t d = (uint64_t)L[i] - r[i] - bw;
    w[i] = flip ? (uint32_t)d : r[i];
    bw = (uint32_t)(d >> 63);
  }
}

/* [|u|](T_A) + [|v|](T_R), digit strings pre-shifted so that digit nwin-1
   sits in the top nibble; u_neg / v_neg flip every digit's sign (the tables
   hold -A, -R).  Leaves the completed sum of the last addition in t. */
FDG_DEV void hs_chain(ge_p1p1 &t, uint32_t (&ud)[5], uint32_t (&vd)[5], bool u_neg, bool v_neg, uint32_t nwin,
                      const uint32_t *wsl, const uint32_t *ta) {
  const uint32_t *tr = tab_r(const_cast<uint32_t *>(wsl));
  __shared__ uint32_t s_stage[FDGPU_BLOCK / 64][2][FDGPU_STAGE_WAVE_WORDS];
  static_assert(sizeof(s_stage) == FDGPU_STAGE_LDS, "FDGPU_SPREAD_LDS is derived from this");
  uint32_t *st_r = &s_stage[threadIdx.x >> 6][0][0];
  uint32_t *st_a = &s_stage[threadIdx.x >> 6][1][0];
  ge_p2 acc2;
  ge_p3 acc3;
  uint32_t q[40];
  {                                             /* top window: O + T_A[du] + T_R[dv] */
    const int du = sext4(ud[4] >> 28), dv = sext4(vd[4] >> 28);
    shl4_5(ud); shl4_5(vd);
    /* the entry as a p3 point needs T = XY/Z (its 2dT would need 1/d): add
       it to the identity instead */
    atab_load(q, ta, du);
    ge_p3_0(acc3);
    ge_add_cached_regs(t, acc3, q, (du < 0) != u_neg);
    ge_p1p1_to_p3(acc3, t);
    atab_load(q, tr, dv);
    ge_add_cached_regs(t, acc3, q, (dv < 0) != v_neg);
  }
#pragma unroll 1
  for (uint32_t j = 1; j < nwin; j++) {
    ge_p1p1_to_p2(acc2, t);
    const int du = sext4(ud[4] >> 28), dv = sext4(vd[4] >> 28);
    shl4_5(ud); shl4_5(vd);
    stage_entry(st_a, ta, du);
    stage_entry(st_r, tr, dv);
#pragma unroll 1
    for (int r = 0; r < 4; r++) {
      ge_dbl(t, acc2);
      ge_p1p1_to_p2(acc2, t);
    }
    acc3.X = acc2.X; acc3.Y = acc2.Y; acc3.Z = acc2.Z; fe_mul(acc3.T, t.X, t.Y);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   /* the window's LDS-DMA has landed */
    unstage_entry_signed(q, st_a, (du < 0) != u_neg);
    ge_add_cached_regs_swapped(t, acc3, q, (du < 0) != u_neg);
    ge_p1p1_to_p3(acc3, t);
    unstage_entry_signed(q, st_r, (dv < 0) != v_neg);
    ge_add_cached_regs_swapped(t, acc3, q, (dv < 0) != v_neg);
  }
}

/* ---- the stages the one-lane and the two-lane verify kernels share
   (load32, wave_max_u32 and hram_k: fdgpu_hram.h) ---- */

/* Decode a point, test its order and build the table of its negative's
   multiples at tab (a table's virtual base: tab_a / tab_r).  The verdict is
   kverd's word: bit 0 decoded, bit 1 small order. */
FDG_DEV uint32_t decode_neg_table(uint32_t *tab, const uint32_t (&enc)[8], bool ref_map) {
  ge_p3 P, Pn;
  const bool ok = ge_decode(P, enc, ref_map);
  const bool small = ge_is_small_order_affine(P);
  ge_p3_neg(Pn, P);
  atab_build(tab, Pn);
  return (ok ? 1u : 0u) | (small ? 2u : 0u);
}

/* split k; lanes that need no chain (already failed, or past the batch) run
   no Euclid steps: k = 0 */
FDG_DEV void hs_split_masked(hs_split_t &hs, const uint32_t (&k)[8], bool need) {
  uint32_t ke[8];
#pragma unroll
  for (int j = 0; j < 8; j++) ke[j] = need ? k[j] : 0u;
  hs_split(hs, ke);
}

/* the radix-16 digits of |u| and |v|; returns the lane's digit count (>= 1) */
FDG_DEV uint32_t hs_digits(uint32_t (&ud)[5], uint32_t (&vd)[5], const hs_split_t &hs) {
  uint32_t ndu = 0, ndv = 0;
  recode16_160(ud, ndu, hs.u);
  recode16_160(vd, ndv, hs.v);
  return max(max(ndu, ndv), 1u);
}

/* the comb's scalar: w = v S mod L of a half-size lane, else S ([S]B for the
   full-length path; 0 for a lane already failed) */
FDG_DEV void comb_scalar(uint32_t (&w)[8], const hs_split_t &hs, const uint32_t (&S)[8], bool half) {
  hs_wscalar(w, hs.v, hs.v_neg, S);
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = half ? w[j] : S[j];
}

/* a full-path lane leaves k's digits for fdgpu_full_kernel */
FDG_DEV void park_full(uint32_t *park, const uint32_t (&k)[8]) {
  uint32_t kd[KD_WORDS];
  sc_recode16(kd, k);
#pragma unroll
  for (int j = 0; j < KD_WORDS; j++) park[HPARK_KD + j] = kd[j];
  park[HPARK_CODE] = 0u;
}

/* append signature i of every lane with q_full to the fallback queue (rare):
   one atomic per wave, ballot-compacted */
FDG_DEV void queue_full_lanes(uint32_t *queue, uint32_t *queue_cnt, bool q_full, uint32_t i) {
  const uint64_t m = __ballot(q_full);
  if (m) {
    const int lane = (int)(threadIdx.x & 63u);
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(queue_cnt, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, 64);
    if (q_full) queue[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
  }
}

/* The verify kernel of the half-size path; codes of lanes it settles are
   written here, lanes whose split failed are queued for fdgpu_full_kernel.
   The body takes its block index: the merged launch (fdgpu_verify_hs_multi_kernel)
   runs it for the batch blockIdx.y names.  PH (prehashed, the synchronous
   API's messages too large for one arena): the descriptor's msg_off holds
   the lane's SHA-512(R || A || M) state words, hashed beforehand in pieces
   by fdgpu_sha512_stream_kernel; the product instantiations have PH false.
   The hash reduction, the S < L gate, the decodes with decode2's error order,
   nb's wave maximum and the final check are written out here and again in
   fdgpu_verify_pair_kernel: as calls to shared helpers they changed this
   kernel's register allocation (256 VGPRs, 68 B of scratch per lane). */
template <bool KC, bool PH = false>
FDG_DEV void verify_hs_body(const uint8_t *__restrict__ arena, const fdgpu_sig_desc_t *__restrict__ sigs, uint32_t n_sig_arg,
                            const uint32_t *__restrict__ n_sig_dev, const uint32_t *__restrict__ btab,
                            uint32_t *__restrict__ ws, const uint32_t *__restrict__ perm, int8_t *__restrict__ codes,
                            uint32_t *__restrict__ queue, uint32_t *__restrict__ queue_cnt, uint32_t flags,
                            const uint32_t *__restrict__ key_of, const uint32_t *__restrict__ kverd, uint32_t bx) {
  /* n_sig_dev: the count is produced on the device (GPU-side ingest) and the
     grid covers an upper bound; blocks past it leave at once */
  const uint32_t n_sig = n_sig_dev ? *n_sig_dev : n_sig_arg;
  if (bx * blockDim.x >= n_sig) return;
  const uint32_t i = bx * blockDim.x + threadIdx.x;
  const bool active = i < n_sig;
  const bool ref_map = (flags & FDGPU_FLAG_REF_MAP) != 0;
  const fdgpu_sig_desc_t d = sigs[active ? i : n_sig - 1];
  uint32_t nb = sha512_hram_blocks(d.msg_sz);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nb = max(nb, (uint32_t)__shfl_xor((int)nb, off));
  uint32_t *wsl = lane_ws(ws, i);
  uint32_t *aux = lane_aux(queue, i);
  const uint32_t *ta = tab_a(wsl);             /* this lane's -A table */
  FDGPU_STAMP(0);
  uint32_t Renc[8], Aenc[8];
  load32(Renc, arena + d.sig_off);
  load32(Aenc, arena + d.pub_off);
  /* k = SHA-512(R || A || M) mod L */
  uint32_t k[8];
  {
    uint64_t h[8];
    if (PH) {
#pragma unroll
      for (int j = 0; j < 8; j++) h[j] = ((const uint64_t *)(arena + d.msg_off))[j];
    } else {
      sha512_hram(h, Renc, Aenc, arena + d.msg_off, d.msg_sz, nb);
    }
    FDGPU_STAMP(1);
    uint32_t kx[16];
#pragma unroll
    for (int j = 0; j < 8; j++) { kx[2 * j] = bswap32((uint32_t)(h[j] >> 32)); kx[2 * j + 1] = bswap32((uint32_t)h[j]); }
    sc_reduce512(k, kx);
  }
  /* step 1: S < L (fd_ed25519_user.c:159-161) */
  uint32_t S[8];
  load32(S, arena + d.sig_off + 32);
  int code = sc_lt_L(S) ? 0 : -1;
#pragma unroll
  for (int j = 0; j < 8; j++) S[j] = code ? 0u : S[j];
  FDGPU_STAMP(2);
  /* step 2: decode A then R (decode2 reports A first), small-order tests,
     tables of -A and -R */
  {
    ge_p3 P, Pn;
    bool a_ok, a_small;
    if (KC) {
      /* key cache: the -A table was built once per distinct key by
         fdgpu_key_table_kernel in its representative lane's workspace, and
         the chain reads it there */
      const uint32_t di = active ? i : n_sig - 1u, r = key_of[di], vd = kverd[r];
      a_ok = (vd & 1u) != 0;
      a_small = (vd & 2u) != 0;
      ta = tab_a(lane_ws(ws, r));
    } else {
      a_ok = ge_decode(P, Aenc, ref_map);
      a_small = ge_is_small_order_affine(P);
      ge_p3_neg(Pn, P);
      atab_build(tab_a(wsl), Pn);
    }
    FDGPU_STAMP(3);
    const bool r_ok = ge_decode(P, Renc, ref_map);
    const bool r_small = ge_is_small_order_affine(P);
    ge_p3_neg(Pn, P);
    atab_build(tab_r(wsl), Pn);
    if (code == 0 && !a_ok) code = ref_map ? -2 : -1;
    if (code == 0 && !r_ok) code = -1;
    if (code == 0 && a_small) code = -2;                 /* fd_ed25519_user.c:194-199 */
    if (code == 0 && r_small) code = -1;
  }
  FDGPU_STAMP(4);
  const bool need = active && code == 0;
  /* split k (lanes already failed run no Euclid steps: k = 0) */
  hs_split_t hs;
  hs_split_masked(hs, k, need);
  uint32_t ud[5], vd[5];
  const uint32_t nd_lane = hs_digits(ud, vd, hs);
  const bool full = need && (!hs.ok || nd_lane > HS_MAX_WIN || (flags & FDGPU_FLAG_KFULL));
  const bool half = need && !full;
  FDGPU_STAMP(5);
  /* [w]B (w = v S mod L), or [S]B for the full-length path; parked cached */
  {
    uint32_t w[8];
    comb_scalar(w, hs, S, half);
    ge_p3 WB;
    comb_sb(WB, w, btab);
    ge_cached c; ge_p3_to_cached(c, WB);
    sb_store(aux, c);
  }
  if (full) park_full(aux + FDGPU_AUX_PARK, k);
  FDGPU_STAMP(6);
  bool eq = false;
  if (__any(half)) {
    /* the wave's digit count; every lane runs it (shorter strings lead with zeros) */
    const uint32_t nwin = wave_max_u32(half ? nd_lane : 1u);
#pragma unroll 1
    for (uint32_t s = nwin; s < 40; s++) { shl4_5(ud); shl4_5(vd); }
    ge_p1p1 t;
    hs_chain(t, ud, vd, hs.u_neg, hs.v_neg, nwin, wsl, ta);
    /* chain == -[w]B:  x = X/Z = -(YpX - YmX)/Z2,  y = Y/T = (YpX + YmX)/Z2 */
    uint32_t q[40];
    sb_load(q, aux);
    fe ypx, ymx, z2, xw, yw, l1, l2;
#pragma unroll
    for (int j = 0; j < 10; j++) { ypx.v[j] = q[j]; ymx.v[j] = q[10 + j]; z2.v[j] = q[20 + j]; }
    fe_sub(xw, ypx, ymx);
    fe_add(yw, ypx, ymx);
    fe_mul(l1, t.X, z2);
    fe_mul(l2, t.Z, xw);
    fe_add(l1, l1, l2);
    const bool ex = fe_iszero(l1);
    fe_mul(l1, t.Y, z2);
    fe_mul(l2, t.T, yw);
    fe_sub(l1, l1, l2);
    eq = ex && fe_iszero(l1);
  }
  FDGPU_STAMP(7);
  if (active && !full) codes[out_idx(perm, i)] = (int8_t)(code ? code : (eq ? 0 : -3));
  queue_full_lanes(queue, queue_cnt, full, i);
}

template <bool KC, bool PH = false>
__global__ void __launch_bounds__(FDGPU_BLOCK, FDGPU_VERIFY_WAVES)
fdgpu_verify_hs_kernel(const uint8_t *__restrict__ arena, const fdgpu_sig_desc_t *__restrict__ sigs, uint32_t n_sig_arg,
                       const uint32_t *__restrict__ n_sig_dev, const uint32_t *__restrict__ btab,
                       uint32_t *__restrict__ ws, const uint32_t *__restrict__ perm, int8_t *__restrict__ codes,
                       uint32_t *__restrict__ queue, uint32_t *__restrict__ queue_cnt, uint32_t flags,
                       const uint32_t *__restrict__ key_of, const uint32_t *__restrict__ kverd) {
  verify_hs_body<KC, PH>(arena, sigs, n_sig_arg, n_sig_dev, btab, ws, perm, codes, queue, queue_cnt, flags, key_of,
                         kverd, blockIdx.x);
}

/* SHA-512(R_i || A_i || M) of one message shared by n <= 64 signatures (lane
   i: signature i), over blocks [blk0, blk0 + nblk) of the n streams, in a
   launch per piece of M: the synchronous API's messages too large for one
   arena.  state: n x 8 words (initialised by the launch with blk0 == 0),
   left as sha512_hram leaves its h.  mbuf holds M[m0, m0 + mlen): every
   message byte of the launch's blocks (the host's piece).  Block b of a
   stream is R || A || M[0, 64) for b = 0 and M[128 b - 64, 128 b + 64)
   after, padded past msg_sz and length-terminated as sha512_hram does;
   bytes are gathered one by one (a rare path, one wave). */
__global__ void __launch_bounds__(64) fdgpu_sha512_stream_kernel(const uint8_t *__restrict__ mbuf, uint64_t m0,
                                                                 uint64_t mlen, uint64_t msg_sz, uint64_t blk0,
                                                                 uint32_t nblk, const uint8_t *__restrict__ ra,
                                                                 uint64_t *__restrict__ state, uint32_t n) {
  const uint32_t i = threadIdx.x;
  if (i >= n) return;
  const uint64_t H0[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL,
                          0xa54ff53a5f1d36f1ULL, 0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL,
                          0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
  uint64_t h[8];
  for (int j = 0; j < 8; j++) h[j] = blk0 ? state[8 * i + j] : H0[j];
  const uint64_t total = (64u + msg_sz + 16u) / 128u + 1u, bitlen = (64u + msg_sz) * 8u;
  for (uint64_t b = blk0; b < blk0 + nblk; b++) {
    uint64_t w[16];
    for (int t = 0; t < 16; t++) {
      uint64_t v = 0;
      for (int j = 0; j < 8; j++) {
        const uint64_t s = 128u * b + 8u * (uint64_t)t + (uint64_t)j;     /* position in R || A || M */
        uint32_t byte;
        if (s < 64u) {
          byte = ra[64u * i + s];
        } else {
          const uint64_t g = s - 64u;                                     /* position in M */
          byte = g < msg_sz ? (g >= m0 && g < m0 + mlen ? mbuf[g - m0] : 0u) : g == msg_sz ? 0x80u : 0u;
        }
        v = (v << 8) | byte;
      }
      w[t] = v;
    }
    if (b + 1 == total) { w[14] = 0; w[15] = bitlen; }
    sha512_compress(h, w);
  }
  for (int j = 0; j < 8; j++) state[8 * i + j] = h[j];
}

/* Several batches' verifies as ONE launch (FDGPU_FLAG_MERGE): block (x, y)
   is block x of batch y.  Concurrent 16 K-signature launches from separate
   streams share the CUs badly -- eight 8 K launches at once take 1.33 ms,
   one 64 K launch 0.85 ms (profiles/r04/conc_probe.jsonl) -- so an engine
   with several batches ready verifies them together. */
__global__ void __launch_bounds__(FDGPU_BLOCK, FDGPU_VERIFY_WAVES)
fdgpu_verify_hs_multi_kernel(const fdgpu_mbatch_t *__restrict__ mb, const uint32_t *__restrict__ btab, uint32_t flags) {
  const fdgpu_mbatch_t b = mb[blockIdx.y];
  if (blockIdx.x * blockDim.x >= b.bound) return;
  verify_hs_body<false>(b.arena, b.sigs, b.bound, b.n_sig, btab, b.ws, nullptr, b.codes, b.queue, b.cnt, flags, nullptr,
                        nullptr, blockIdx.x);
}

/* ---------------- two lanes per signature (FDGPU_FLAG_KPAIR) ----------------
   The same equation as fdgpu_verify_hs_kernel, with the work of one
   signature split over two adjacent lanes of a wave, for batches too small
   to fill the GPU's wave slots (a lone wave's lifetime is then the batch's
   latency).  Lane 2i (the A lane) decodes A and builds the -A table while
   lane 2i+1 (the R lane) decodes R and builds the -R table: one
   exponentiation per lane instead of two.  Each lane then runs a chain over
   its own half-size scalar -- [|u|](+-A) or [|v|](+-R), 4 doublings and ONE
   addition per window -- and the two sums are exchanged across the pair and
   added, so both lanes hold the complete [u](-A) + [v](-R) for the check
   against -[w]B.  SHA-512, the split and the comb run in both lanes (SIMT:
   it costs the wave the same time as running them in one).  Per signature
   the pair does ~1.4x the work of one lane; per wave it finishes ~30%
   sooner.  Lanes whose split fails are queued by their A lane for
   fdgpu_full_kernel exactly as the one-lane kernel queues them (the A
   table, the parked R, k's digits and [S]B are in the signature's own
   workspace). */

/* [|d|](+-T) for one table, digits pre-shifted so that digit nwin-1 sits in
   the top nibble; staged through LDS like hs_chain (one entry per window). */
FDG_DEV void hs_chain1(ge_p1p1 &t, uint32_t (&dd)[5], bool neg, uint32_t nwin, const uint32_t *tab) {
  __shared__ uint32_t s_stage1[FDGPU_BLOCK / 64][FDGPU_STAGE_WAVE_WORDS];
  static_assert(sizeof(s_stage1) == FDGPU_STAGE_LDS_PAIR, "FDGPU_SPREAD_LDS_PAIR is derived from this");
  uint32_t *st = &s_stage1[threadIdx.x >> 6][0];
  ge_p2 acc2;
  ge_p3 acc3;
  uint32_t q[40];
  {                                             /* top window: O + T[d] */
    const int d = sext4(dd[4] >> 28);
    shl4_5(dd);
    atab_load(q, tab, d);
    ge_p3_0(acc3);
    ge_add_cached_regs(t, acc3, q, (d < 0) != neg);
  }
#pragma unroll 1
  for (uint32_t j = 1; j < nwin; j++) {
    ge_p1p1_to_p2(acc2, t);
    const int d = sext4(dd[4] >> 28);
    shl4_5(dd);
    stage_entry(st, tab, d);
#pragma unroll 1
    for (int r = 0; r < 4; r++) {
      ge_dbl(t, acc2);
      ge_p1p1_to_p2(acc2, t);
    }
    acc3.X = acc2.X; acc3.Y = acc2.Y; acc3.Z = acc2.Z; fe_mul(acc3.T, t.X, t.Y);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   /* the window's LDS-DMA has landed */
    unstage_entry_signed(q, st, (d < 0) != neg);
    ge_add_cached_regs_swapped(t, acc3, q, (d < 0) != neg);
  }
}

FDG_DEV void fe_xchg_pair(fe &r, const fe &a) {
#pragma unroll
  for (int j = 0; j < 10; j++) r.v[j] = (uint32_t)__shfl_xor((int)a.v[j], 1);
}

/* PH: k from the lane's SHA-512 state words at msg_off, as in verify_hs_body
   (the chain diagnostic's instantiation; the product's has PH false) */
template <bool PH = false>
__global__ void __launch_bounds__(FDGPU_BLOCK, FDGPU_VERIFY_WAVES)
fdgpu_verify_pair_kernel(const uint8_t *__restrict__ arena, const fdgpu_sig_desc_t *__restrict__ sigs, uint32_t n_sig_arg,
                         const uint32_t *__restrict__ n_sig_dev, const uint32_t *__restrict__ btab,
                         uint32_t *__restrict__ ws, const uint32_t *__restrict__ perm, int8_t *__restrict__ codes,
                         uint32_t *__restrict__ queue, uint32_t *__restrict__ queue_cnt, uint32_t flags) {
  const uint32_t n_sig = n_sig_dev ? *n_sig_dev : n_sig_arg;
  if (blockIdx.x * (blockDim.x / 2u) >= n_sig) return;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x, i = g >> 1;
  const bool rl = (g & 1u) != 0;                /* the R lane of signature i (else its A lane) */
  const bool active = i < n_sig;
  const bool ref_map = (flags & FDGPU_FLAG_REF_MAP) != 0;
  const fdgpu_sig_desc_t d = sigs[active ? i : n_sig - 1];
  const uint32_t nb = wave_max_u32(sha512_hram_blocks(d.msg_sz));
  uint32_t *wsl = lane_ws(ws, i);             /* i < the workspace's lanes: ceil(n / 128) x 128 <= ceil(n / 256) x 256 */
  uint32_t *aux = lane_aux(queue, i);
  uint32_t *tab = rl ? tab_r(wsl) : tab_a(wsl);                 /* the lane's own table */
  uint32_t Renc[8], Aenc[8];
  load32(Renc, arena + d.sig_off);
  load32(Aenc, arena + d.pub_off);
  uint32_t k[8];
  if (PH) {
    uint32_t kx[16];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t h = ((const uint64_t *)(arena + d.msg_off))[j];
      kx[2 * j] = bswap32((uint32_t)(h >> 32)); kx[2 * j + 1] = bswap32((uint32_t)h);
    }
    sc_reduce512(k, kx);
  } else {
    hram_k(k, Renc, Aenc, arena, d, nb);
  }
  uint32_t S[8];
  load32(S, arena + d.sig_off + 32);
  int code = sc_lt_L(S) ? 0 : -1;
#pragma unroll
  for (int j = 0; j < 8; j++) S[j] = code ? 0u : S[j];
  /* each lane decodes its own point and builds its table */
  {
    uint32_t enc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) enc[j] = rl ? Renc[j] : Aenc[j];
    /* both verdicts in both lanes, in decode2's order (A first) */
    const uint32_t mine = decode_neg_table(tab, enc, ref_map);
    const uint32_t other = (uint32_t)__shfl_xor((int)mine, 1);
    const uint32_t av = rl ? other : mine, rv = rl ? mine : other;
    if (code == 0 && !(av & 1u)) code = ref_map ? -2 : -1;
    if (code == 0 && !(rv & 1u)) code = -1;
    if (code == 0 && (av & 2u)) code = -2;                 /* fd_ed25519_user.c:194-199 */
    if (code == 0 && (rv & 2u)) code = -1;
  }
  const bool need = active && code == 0;
  hs_split_t hs;
  hs_split_masked(hs, k, need);
  uint32_t ud[5], vd[5];
  const uint32_t nd_lane = hs_digits(ud, vd, hs);
  const bool full = need && (!hs.ok || nd_lane > HS_MAX_WIN || (flags & FDGPU_FLAG_KFULL));
  const bool half = need && !full;
  {
    uint32_t w[8];
    comb_scalar(w, hs, S, half);
    /* the A lane sums the comb's low tables, the R lane its high ones; the
       halves are exchanged and added */
    ge_p3 WB, WBo;
    comb_sb(WB, w, btab, rl ? BC_NDIG / 2u : 0u, rl ? BC_NDIG : BC_NDIG / 2u);
    fe_xchg_pair(WBo.X, WB.X);
    fe_xchg_pair(WBo.Y, WB.Y);
    fe_xchg_pair(WBo.Z, WB.Z);
    fe_xchg_pair(WBo.T, WB.T);
    ge_cached c; ge_p3_to_cached(c, WBo);
    ge_p1p1 tw; ge_add_cached(tw, WB, c, false);
    ge_p1p1_to_p3(WB, tw);
    ge_p3_to_cached(c, WB);
    if (!rl) sb_store(aux, c);
  }
  if (full && !rl) park_full(aux + FDGPU_AUX_PARK, k);
  bool eq = false;
  if (__any(half)) {
    const uint32_t nwin = wave_max_u32(half ? nd_lane : 1u);
    uint32_t dd[5];
#pragma unroll
    for (int j = 0; j < 5; j++) dd[j] = rl ? vd[j] : ud[j];
#pragma unroll 1
    for (uint32_t s2 = nwin; s2 < 40; s2++) shl4_5(dd);
    ge_p1p1 t;
    hs_chain1(t, dd, rl ? hs.v_neg : hs.u_neg, nwin, tab);
    /* exchange the halves and add: both lanes hold [u](-A) + [v](-R) */
    ge_p3 mine, other;
    ge_p1p1_to_p3(mine, t);
    fe_xchg_pair(other.X, mine.X);
    fe_xchg_pair(other.Y, mine.Y);
    fe_xchg_pair(other.Z, mine.Z);
    fe_xchg_pair(other.T, mine.T);
    ge_cached oc;
    ge_p3_to_cached(oc, other);
    ge_add_cached(t, mine, oc, false);
    /* chain == -[w]B (the A lane parked [w]B; a lane reads its own pair's entry) */
    uint32_t q[40];
    sb_load(q, aux);
    fe ypx, ymx, z2, xw, yw, l1, l2;
#pragma unroll
    for (int j = 0; j < 10; j++) { ypx.v[j] = q[j]; ymx.v[j] = q[10 + j]; z2.v[j] = q[20 + j]; }
    fe_sub(xw, ypx, ymx);
    fe_add(yw, ypx, ymx);
    fe_mul(l1, t.X, z2);
    fe_mul(l2, t.Z, xw);
    fe_add(l1, l1, l2);
    const bool ex = fe_iszero(l1);
    fe_mul(l1, t.Y, z2);
    fe_mul(l2, t.T, yw);
    fe_sub(l1, l1, l2);
    eq = ex && fe_iszero(l1);
  }
  if (active && !full && !rl) codes[out_idx(perm, i)] = (int8_t)(code ? code : (eq ? 0 : -3));
  queue_full_lanes(queue, queue_cnt, full && !rl, i);
}

/* ---------------- key cache (FDGPU_FLAG_KCACHE) ----------------
   Signers repeat within a batch (a vote account signs every slot).  Each
   distinct public key is decoded and its -A table built once, in the
   workspace of one representative lane; the verify and fallback kernels'
   other lanes with that key read that table in place instead of
   decompressing A (a 2^252-3 exponentiation) and building their own.
   Results are unchanged: the decode is a function of the 32 key bytes only.

   fdgpu_key_dedup_kernel: an open-addressing table of signature indices,
   keyed by a seeded hash of all 32 key bytes.  A lane claims an empty slot
   with atomicCAS (after a plain load saw it empty), or compares its key with
   the bytes of the index a slot already holds (the arena is immutable, so
   nothing waits on another lane).  After KC_PROBES probes it stays its own
   representative, which bounds the work whatever keys a batch carries.  key_of[i] = representative of i;
   the representatives are appended to reps (compact, so the table kernel
   runs dense waves however they are scattered over the batch). */
#define KC_PROBES 32u
#define KC_EMPTY 0xffffffffu

FDG_DEV uint32_t kc_hash(const uint32_t (&a)[8], uint64_t seed) {
  uint64_t h = seed;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    h ^= ((uint64_t)a[2 * j + 1] << 32) | a[2 * j];
    h *= 0x9e3779b97f4a7c15ull;
    h ^= h >> 29;
  }
  h *= 0xbf58476d1ce4e5b9ull;
  return (uint32_t)(h >> 32) ^ (uint32_t)h;
}

__global__ void __launch_bounds__(256) fdgpu_key_dedup_kernel(const uint8_t *__restrict__ arena,
                                                              const fdgpu_sig_desc_t *__restrict__ sigs,
                                                              uint32_t n_sig_arg, const uint32_t *__restrict__ n_sig_dev,
                                                              uint32_t *__restrict__ ht, uint32_t ht_mask,
                                                              uint32_t *__restrict__ key_of, uint32_t *__restrict__ reps,
                                                              uint32_t *__restrict__ rep_cnt, uint64_t seed) {
  const uint32_t n_sig = n_sig_dev ? *n_sig_dev : n_sig_arg;
  if (blockIdx.x * blockDim.x >= n_sig) return;     /* whole block: the barriers below need every thread */
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool is_rep = false;
  if (i < n_sig) {
    uint32_t a[8];
    load32(a, arena + sigs[i].pub_off);
    uint32_t slot = kc_hash(a, seed) & ht_mask, rep = i;
    for (uint32_t p = 0; p < KC_PROBES; p++, slot = (slot + 1u) & ht_mask) {
      /* a plain load first: a signer's slot is taken by its first signature,
         and the many later ones then compare without an atomic on a hot line */
      uint32_t v = ht[slot];                        /* stale only as EMPTY: the CAS then reads it */
      if (v == KC_EMPTY) {
        v = atomicCAS(&ht[slot], KC_EMPTY, i);
        if (v == KC_EMPTY) break;                   /* claimed: i represents its key */
      }
      uint32_t b[8];
      load32(b, arena + sigs[v].pub_off);
      uint32_t diff = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) diff |= a[j] ^ b[j];
      if (!diff) { rep = v; break; }
    }
    key_of[i] = rep;
    is_rep = rep == i;
  }
  /* append the representatives: wave offsets in LDS, one global atomic per
     workgroup (a single counter takes every one of them) */
  __shared__ uint32_t s_cnt, s_base;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const uint64_t m = __ballot(is_rep);
  const int lane = (int)(threadIdx.x & 63u);
  uint32_t wbase = 0;
  if (m && lane == __ffsll((long long)m) - 1) wbase = atomicAdd(&s_cnt, (uint32_t)__popcll(m));
  if (m) wbase = (uint32_t)__shfl((int)wbase, __ffsll((long long)m) - 1, 64);
  __syncthreads();
  if (threadIdx.x == 0) s_base = s_cnt ? atomicAdd(rep_cnt, s_cnt) : 0u;
  __syncthreads();
  if (is_rep) reps[s_base + wbase + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
}

/* One lane per representative: decode A, small-order test, -A table into the
   representative's own workspace, verdict (bit 0 decoded, bit 1 small
   order) into kverd.  The grid covers every signature; blocks past the
   representative count leave at once. */
__global__ void __launch_bounds__(FDGPU_BLOCK, FDGPU_VERIFY_WAVES)
fdgpu_key_table_kernel(const uint8_t *__restrict__ arena, const fdgpu_sig_desc_t *__restrict__ sigs,
                       uint32_t *__restrict__ ws, const uint32_t *__restrict__ reps,
                       const uint32_t *__restrict__ rep_cnt, uint32_t *__restrict__ kverd, uint32_t flags) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= *rep_cnt) return;
  const uint32_t i = reps[q];
  uint32_t Aenc[8];
  load32(Aenc, arena + sigs[i].pub_off);
  kverd[i] = decode_neg_table(tab_a(lane_ws(ws, i)), Aenc, (flags & FDGPU_FLAG_REF_MAP) != 0);
}

/* The queued lanes of fdgpu_verify_hs_kernel: [S]B + [k](-A) with k's 64
   windows (dsm_k), compared with the decoded R (from the lane's -R table). */
__global__ void __launch_bounds__(FDGPU_BLOCK, FDGPU_VERIFY_WAVES)
fdgpu_full_kernel(uint32_t *__restrict__ ws, const uint32_t *__restrict__ perm, int8_t *__restrict__ codes,
                  const uint32_t *__restrict__ queue, const uint32_t *__restrict__ queue_cnt, uint32_t slots,
                  const uint32_t *__restrict__ key_of);

FDG_DEV void full_body(uint32_t *__restrict__ ws, const uint32_t *__restrict__ perm, int8_t *__restrict__ codes,
                       const uint32_t *__restrict__ queue, const uint32_t *__restrict__ queue_cnt, uint32_t slots,
                       const uint32_t *__restrict__ key_of, uint32_t bx) {
  const uint32_t cnt = *queue_cnt;
  if (bx * blockDim.x >= cnt) return;
  for (uint32_t q = bx * blockDim.x + threadIdx.x; q < cnt; q += slots) {
    const uint32_t i = queue[q];
    uint32_t *wsl = lane_ws(ws, i);
    const uint32_t *aux = lane_aux(queue, i), *park = aux + FDGPU_AUX_PARK;
    uint32_t kd[KD_WORDS];
#pragma unroll
    for (int j = 0; j < KD_WORDS; j++) kd[j] = park[HPARK_KD + j];
    ge_p2 Rc;
    dsm_k(Rc, kd, aux, tab_a(key_of ? lane_ws(ws, key_of[i]) : wsl));
    /* == R: the -R table's entry 1 is (Y-X, Y+X, 2Z, -2dT) of R = (X:Y:Z),
       so 2X = YmX - YpX and 2Y = YpX + YmX; compare X / Z, Y / Z crosswise */
    uint32_t er[40];
    atab_load(er, tab_r(wsl), 1);
    fe ypx, ymx, z2, x2, y2, l, r;
#pragma unroll
    for (int j = 0; j < 10; j++) { ypx.v[j] = er[j]; ymx.v[j] = er[10 + j]; z2.v[j] = er[20 + j]; }
    fe_carry(ypx); fe_carry(ymx); fe_carry(z2);
    fe_sub(x2, ymx, ypx);
    fe_add(y2, ypx, ymx);
    fe_mul(l, Rc.X, z2); fe_mul(r, x2, Rc.Z);
    bool eq = fe_eq(l, r);
    fe_mul(l, Rc.Y, z2); fe_mul(r, y2, Rc.Z);
    eq = eq && fe_eq(l, r);
    codes[out_idx(perm, i)] = (int8_t)(eq ? 0 : -3);
  }
}

__global__ void __launch_bounds__(FDGPU_BLOCK, FDGPU_VERIFY_WAVES)
fdgpu_full_kernel(uint32_t *__restrict__ ws, const uint32_t *__restrict__ perm, int8_t *__restrict__ codes,
                  const uint32_t *__restrict__ queue, const uint32_t *__restrict__ queue_cnt, uint32_t slots,
                  const uint32_t *__restrict__ key_of) {
  full_body(ws, perm, codes, queue, queue_cnt, slots, key_of, blockIdx.x);
}

/* the fallback of a merged verify: block (x, y) serves batch y's queue */
__global__ void __launch_bounds__(FDGPU_BLOCK, FDGPU_VERIFY_WAVES)
fdgpu_full_multi_kernel(const fdgpu_mbatch_t *__restrict__ mb) {
  const fdgpu_mbatch_t b = mb[blockIdx.y];
  if (blockIdx.x >= b.slow) return;
  full_body(b.ws, nullptr, b.codes, b.queue, b.cnt, b.slow * FDGPU_BLOCK, nullptr, blockIdx.x);
}

/* Per transaction: fd_ed25519_verify_batch_single_msg's first-error order
   (fd_ed25519_user.c:232-310) over its signatures' codes, plus the batch's
   accept/reject results compacted by wavefront ballot: bit t of accept[]
   is set iff transaction t verified (one 64-bit word per wave; the verify
   tile only needs accept/reject, so it can read n/8 bytes instead of n). */
__global__ void __launch_bounds__(256) fdgpu_combine_kernel(const fdgpu_txn_desc_t *__restrict__ txns, uint32_t n_txn,
                                                            const int8_t *__restrict__ sig_codes,
                                                            int8_t *__restrict__ txn_codes,
                                                            uint64_t *__restrict__ accept) {
  /* FDGPU_AUX_BLOCKS blocks stride over the batch, 256 txns a step */
  for (uint32_t t0 = blockIdx.x * blockDim.x; t0 < n_txn; t0 += gridDim.x * blockDim.x) {
    const uint32_t t = t0 + threadIdx.x;
    int code = -1;
    if (t < n_txn) {
      const fdgpu_txn_desc_t d = txns[t];
      if (d.sig_cnt >= 1 && d.sig_cnt <= 16) {             /* else ERR_SIG (fd_ed25519_user.c:238-241) */
        int first_struct = 0, any_msg = 0;
        for (uint32_t j = 0; j < d.sig_cnt; j++) {
          const int c = sig_codes[d.sig0 + j];
          if (c == -3) any_msg = 1;
          else if (c != 0 && first_struct == 0) first_struct = c;
        }
        /* pass 1 reports its first failure before any pass-2 (equation) failure */
        code = first_struct ? first_struct : (any_msg ? -3 : 0);
      }
      txn_codes[t] = (int8_t)code;
    }
    const uint64_t ok = __ballot(t < n_txn && code == 0);   /* every lane of the wave takes part */
    if (accept && (threadIdx.x & 63u) == 0 && t < n_txn) accept[t >> 6] = ok;
  }
}

}  // namespace

extern "C" {

char const *fdgpu_kernel_path(void) { return "halfsize: fdgpu_verify_hs_kernel + fdgpu_full_kernel"; }

/* every compile-time switch of the kernels, as JSON members; the return
   value is 1 iff each is at the shipped default (fdgpu_build_info) */
int fdgpu_kernel_build_info(char *buf, size_t n) {
  snprintf(buf, n, "\"verify_waves\":%d,\"atab_words\":%u,\"phase_stamps\":%d", (int)FDGPU_VERIFY_WAVES,
           (unsigned)FDGPU_ATAB_WORDS, (int)FDGPU_PHASE_STAMPS);
  return FDGPU_VERIFY_WAVES == 2 && FDGPU_ATAB_WORDS == 40u && FDGPU_PHASE_STAMPS == 0;
}

hipError_t fdgpu_verify_occupancy(int *blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, fdgpu_verify_hs_kernel<false>, FDGPU_BLOCK, 0);
}

size_t fdgpu_ws_bytes(uint64_t n_sig) { return fdgpu_ws_layout(nullptr, n_sig).bytes; }

hipError_t fdgpu_launch_verify_sigs(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_sigs, uint32_t n_sig,
                                    const uint32_t *d_perm, const uint32_t *d_btab, uint32_t *d_ws,
                                    int8_t *d_sig_codes, uint32_t flags, hipStream_t stream, const uint32_t *d_n_sig,
                                    uint32_t resident_blocks, uint64_t kc_seed, int cnt_zeroed) {
  if (!n_sig) return hipSuccess;
  const uint32_t grid = (n_sig + FDGPU_BLOCK - 1) / FDGPU_BLOCK;
  const fdgpu_ws_layout_t l = fdgpu_ws_layout(d_ws, n_sig);
  hipError_t e = cnt_zeroed ? hipSuccess : hipMemsetAsync(l.cnt, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  /* the queued full-length lanes get as many blocks as the batch's grid could
     keep resident (all of them, up to every wave slot of the GPU: the
     engine's occupancy x CUs), each exiting at once when the queue holds
     nothing for it */
  if (!resident_blocks) resident_blocks = 1;
  uint32_t slow_blocks = grid < resident_blocks ? grid : resident_blocks;
  /* strides over its queue; a tile-sized batch (<= 64 blocks) gets a quarter */
  const uint32_t slow_cap = grid > 64u ? FDGPU_FULL_BLOCKS : FDGPU_FULL_BLOCKS / 4u;
  if (slow_blocks > slow_cap) slow_blocks = slow_cap;
  const uint32_t *key_of = nullptr;
  if (flags & FDGPU_FLAG_KCACHE) {
    e = hipMemsetAsync(l.ht, 0xff, l.ht_slots * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(l.rep_cnt, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fdgpu_key_dedup_kernel, dim3((n_sig + 255) / 256), dim3(256), 0, stream, d_arena, d_sigs, n_sig,
                       d_n_sig, l.ht, (uint32_t)(l.ht_slots - 1), l.key_of, l.reps, l.rep_cnt, kc_seed);
    hipLaunchKernelGGL(fdgpu_key_table_kernel, dim3(grid), dim3(FDGPU_BLOCK), 0, stream, d_arena, d_sigs, d_ws, l.reps,
                       l.rep_cnt, l.kverd, flags);
    hipLaunchKernelGGL(fdgpu_verify_hs_kernel<true>, dim3(grid), dim3(FDGPU_BLOCK), 0, stream, d_arena, d_sigs, n_sig,
                       d_n_sig, d_btab, d_ws, d_perm, d_sig_codes, l.queue, l.cnt, flags, l.key_of, l.kverd);
    key_of = l.key_of;
  } else if (flags & FDGPU_FLAG_KPAIR) {
    const uint32_t pgrid = (2u * n_sig + FDGPU_BLOCK - 1) / FDGPU_BLOCK;     /* two lanes per signature */
    hipLaunchKernelGGL(fdgpu_verify_pair_kernel<false>, dim3(pgrid), dim3(FDGPU_BLOCK),
                       (flags & FDGPU_FLAG_KSPREAD) ? FDGPU_SPREAD_LDS_PAIR : 0, stream, d_arena, d_sigs, n_sig,
                       d_n_sig, d_btab, d_ws, d_perm, d_sig_codes, l.queue, l.cnt, flags);
  } else {
    hipLaunchKernelGGL(fdgpu_verify_hs_kernel<false>, dim3(grid), dim3(FDGPU_BLOCK),
                       (flags & FDGPU_FLAG_KSPREAD) ? FDGPU_SPREAD_LDS : 0, stream, d_arena, d_sigs, n_sig,
                       d_n_sig, d_btab, d_ws, d_perm, d_sig_codes, l.queue, l.cnt, flags, nullptr, nullptr);
  }
  hipLaunchKernelGGL(fdgpu_full_kernel, dim3(slow_blocks), dim3(FDGPU_BLOCK), 0, stream, d_ws, d_perm, d_sig_codes,
                     l.queue, l.cnt, slow_blocks * FDGPU_BLOCK, key_of);
  return hipGetLastError();
}

uint64_t fdgpu_sha512_stream_blocks(uint64_t msg_sz) { return (64u + msg_sz + 16u) / 128u + 1u; }

hipError_t fdgpu_launch_sha512_stream(const uint8_t *d_mbuf, uint64_t m0, uint64_t mlen, uint64_t msg_sz,
                                      uint64_t blk0, uint32_t nblk, const uint8_t *d_ra, uint64_t *d_state,
                                      uint32_t n, hipStream_t stream) {
  if (!n || n > 64 || !nblk) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fdgpu_sha512_stream_kernel, dim3(1), dim3(64), 0, stream, d_mbuf, m0, mlen, msg_sz, blk0, nblk,
                     d_ra, d_state, n);
  return hipGetLastError();
}

hipError_t fdgpu_launch_verify_prehashed(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_sigs, uint32_t n_sig,
                                         const uint32_t *d_btab, uint32_t *d_ws, int8_t *d_sig_codes, uint32_t flags,
                                         hipStream_t stream) {
  if (!n_sig) return hipSuccess;
  const uint32_t grid = (n_sig + FDGPU_BLOCK - 1) / FDGPU_BLOCK;
  const fdgpu_ws_layout_t l = fdgpu_ws_layout(d_ws, n_sig);
  hipError_t e = hipMemsetAsync(l.cnt, 0, sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  /* the flags the prehashed kernels read; FDGPU_FLAG_KFULL and FDGPU_FLAG_KPAIR come only from the chain
     diagnostic (fdgpu_debug_verify_prehashed): the synchronous path passes neither */
  const uint32_t kf = flags & (FDGPU_FLAG_REF_MAP | FDGPU_FLAG_KFULL);
  if (flags & FDGPU_FLAG_KPAIR) {
    const uint32_t pgrid = (2u * n_sig + FDGPU_BLOCK - 1) / FDGPU_BLOCK;     /* two lanes per signature */
    hipLaunchKernelGGL(fdgpu_verify_pair_kernel<true>, dim3(pgrid), dim3(FDGPU_BLOCK), 0, stream, d_arena, d_sigs,
                       n_sig, nullptr, d_btab, d_ws, nullptr, d_sig_codes, l.queue, l.cnt, kf);
  } else {
    hipLaunchKernelGGL((fdgpu_verify_hs_kernel<false, true>), dim3(grid), dim3(FDGPU_BLOCK), 0, stream, d_arena, d_sigs,
                       n_sig, nullptr, d_btab, d_ws, nullptr, d_sig_codes, l.queue, l.cnt, kf, nullptr, nullptr);
  }
  hipLaunchKernelGGL(fdgpu_full_kernel, dim3(1), dim3(FDGPU_BLOCK), 0, stream, d_ws, nullptr, d_sig_codes, l.queue,
                     l.cnt, FDGPU_BLOCK, nullptr);
  return hipGetLastError();
}

hipError_t fdgpu_launch_verify_multi(const fdgpu_mbatch_t *mb, uint32_t nb, uint32_t grid_max, uint32_t slow_max,
                                     const uint32_t *d_btab, uint32_t flags, hipStream_t stream) {
  if (!nb || !grid_max) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_verify_hs_multi_kernel, dim3(grid_max, nb), dim3(FDGPU_BLOCK), 0, stream, mb, d_btab, flags);
  hipLaunchKernelGGL(fdgpu_full_multi_kernel, dim3(slow_max ? slow_max : 1, nb), dim3(FDGPU_BLOCK), 0, stream, mb);
  return hipGetLastError();
}

hipError_t fdgpu_launch_combine(const fdgpu_txn_desc_t *d_txns, uint32_t n_txn, const int8_t *d_sig_codes,
                                int8_t *d_txn_codes, uint64_t *d_accept, hipStream_t stream) {
  if (!n_txn) return hipSuccess;
  const uint32_t blocks = (n_txn + 255) / 256;
  hipLaunchKernelGGL(fdgpu_combine_kernel, dim3(blocks < FDGPU_AUX_BLOCKS ? blocks : FDGPU_AUX_BLOCKS), dim3(256), 0,
                     stream, d_txns, n_txn, d_sig_codes, d_txn_codes, d_accept);
  return hipGetLastError();
}

#if FDGPU_PHASE_STAMPS
/* diagnostic builds: copy out the per-wave phase stamps */
int fdgpu_debug_stamps(uint64_t *out, uint64_t n_waves) {
  if (n_waves > FDGPU_STAMP_WAVES) n_waves = FDGPU_STAMP_WAVES;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fdgpu_stamps), n_waves * FDGPU_STAMP_SLOTS * sizeof(uint64_t)) ==
                 hipSuccess ? 0 : -1;
}
#endif

}  // extern "C"
