/* fdt_secp256k1.h -- the secp256k1 precompile's rules as one source for the
   host and the GPU: which instructions of a parsed transaction belong to
   KeccakSecp256k11111111111111111111111111111, how their record tables
   resolve to (signature + recovery id, address, message) triples, what one
   record's check is -- Keccak-256 of the message, ECDSA public-key recovery,
   Keccak-256 of the key, the address compare --, and how the records' codes
   give the transaction's verdict.

   Restates, in the reference's order,
     fd_executor_verify_precompiles  src/flamenco/runtime/fd_executor.c:252-270
     fd_precompile_get_instr_data    src/flamenco/runtime/program/fd_precompiles.c:73-111
     fd_precompile_secp256k1_verify  fd_precompiles.c:212-307
     fd_secp256k1_recover            src/ballet/secp256k1/fd_secp256k1.c:7-45, a wrapper of libsecp256k1 v0.5.0's
                                     secp256k1_ecdsa_recoverable_signature_parse_compact and secp256k1_ecdsa_recover,
                                     whose rules are restated at fdt_secp256k1_recover_core
   The split is fdt_precompile.h's: fdt_secp256k1_walk_core visits the
   records in order, emits each one that resolves and stops emitting at the
   first structural failure; the verdict is fdt_precompile_verdict_core's
   rule over the emitted records' codes (fdt_secp256k1_verdict_core).  Two
   things differ from the Ed25519 walk: a failed resolve is returned as
   fd_precompile_get_instr_data returns it (:261,276,287) -- DATA_OFFSET for
   an instruction index that names no instruction (:97-99), SIGNATURE for
   bytes that leave the instruction's data (:106-108) --, and an index is one
   byte, so there is no "current instruction" form (:88 compares with 0xFFFF).

   The arithmetic is portable C++ over 32-bit limbs, least significant first,
   every product one 32 x 32 -> 64 multiply added to a 64-bit sum that cannot
   overflow ((2^32-1)^2 + 2 (2^32-1) = 2^64-1), which hipcc turns into
   v_mad_u64_u32 and g++ into mul/add/adc.  Field elements
   (mod p = 2^256 - 2^32 - 977) and scalars (mod n) are kept fully reduced
   between operations, so equality is a word compare.  Points are Jacobian
   (X : Y : Z), x = X / Z^2, y = Y / Z^3, infinity Z = 0; the addition
   branches on its special cases (an operand at infinity, equal points,
   opposite points), so every sum the ladder forms is correct.

   Every loop is bounded by a constant: the inversion, the square root and
   the scalar inversion are fixed 256-step square-and-multiply chains over
   public exponents, the ladder is 256 steps, a message is at most
   FDT_SECP256K1_MSG_BLOCKS Keccak blocks.

   Compiled by g++ into libfd_verify_tile.so (fdt_keccak256,
   fdt_secp256k1_recover, fdt_secp256k1_walk, fdt_secp256k1_verdict,
   fdgpu_secp256k1_verify_host) and by hipcc into fdgpu_secp256k1.hip.

   Bounds: as fdt_precompile.h's -- the input is a payload and the fdt_txn_t
   fdt_parse_core made of it; every read is of an account address or of
   instruction data at an offset checked against data_sz first. */
#pragma once

#include <stdint.h>

#include "fdt_keccak256.h"
#include "fdt_precompile.h"

/* ------------------------------------------------------------ multi-limb */

/* r[N + M] = a[N] * b[M] */
template <int N, int M>
FDT_HD void fdt_mp_mul(const uint32_t *a, const uint32_t *b, uint32_t *r) {
  FDT_UNROLL
  for (int i = 0; i < N + M; i++) r[i] = 0;
  FDT_UNROLL
  for (int i = 0; i < N; i++) {
    uint64_t c = 0;
    FDT_UNROLL
    for (int j = 0; j < M; j++) {
      const uint64_t t = (uint64_t)a[i] * b[j] + r[i + j] + c;
      r[i + j] = (uint32_t)t;
      c = t >> 32;
    }
    r[i + M] = (uint32_t)c;
  }
}

template <int A, int B> struct fdt_mp_max { static constexpr int v = A > B ? A : B; };

/* out[max(8, H + K) + 1] = lo[8] + hi[H] * c[K]; it always fits */
template <int H, int K>
FDT_HD void fdt_mp_fold(const uint32_t *lo, const uint32_t *hi, const uint32_t *c, uint32_t *out) {
  constexpr int L = fdt_mp_max<8, H + K>::v + 1;
  uint32_t pr[H + K];
  fdt_mp_mul<H, K>(hi, c, pr);
  uint64_t cy = 0;
  FDT_UNROLL
  for (int i = 0; i < L; i++) {
    const uint64_t t = (uint64_t)(i < 8 ? lo[i] : 0u) + (i < H + K ? pr[i] : 0u) + cy;
    out[i] = (uint32_t)t;
    cy = t >> 32;
  }
}

/* r[8] = t[16] mod m, m = 2^256 - c, c of K limbs below 2^(32 K - 31) (K = 2:
   p, c = 2^32 + 977; K = 5: n, c < 2^129).  2^256 = c (mod m), so the part
   above 2^256 is folded down as hi * c four times, then one conditional
   subtraction.  With v1 = lo + hi c:  v1 < 2^256 (c + 1), so hi1 <= c;
   v2 < 2^256 + c^2, so hi2 <= 1 (K = 2) or < 5 (K = 5); v3 < 2^256 + 5 c,
   so hi3 <= 1, and where it is 1 the low part is below 5 c; v4 = lo3 + hi3 c
   < 2^256.  For K = 2 already v3 < 2^256 and the fourth fold adds 0. */
template <int K>
FDT_HD void fdt_mp_reduce(const uint32_t *t, const uint32_t *c, uint32_t *r) {
  constexpr int L1 = 8 + K + 1, L2 = fdt_mp_max<8, 2 * K + 1>::v + 1, H3 = L2 - 8, L3 = fdt_mp_max<8, H3 + K>::v + 1,
                L4 = fdt_mp_max<8, 1 + K>::v + 1;
  uint32_t a1[L1], a2[L2], a3[L3], a4[L4];
  fdt_mp_fold<8, K>(t, t + 8, c, a1);
  fdt_mp_fold<K + 1, K>(a1, a1 + 8, c, a2);
  fdt_mp_fold<H3, K>(a2, a2 + 8, c, a3);
  fdt_mp_fold<1, K>(a3, a3 + 8, c, a4);
  /* a4 < 2^256 < 2 m: a4 >= m exactly when a4 + c carries out of 2^256, and then a4 - m is that sum's low part */
  uint32_t u[8];
  uint64_t cy = 0;
  FDT_UNROLL
  for (int i = 0; i < 8; i++) {
    const uint64_t s = (uint64_t)a4[i] + (i < K ? c[i] : 0u) + cy;
    u[i] = (uint32_t)s;
    cy = s >> 32;
  }
  FDT_UNROLL
  for (int i = 0; i < 8; i++) r[i] = cy ? u[i] : a4[i];
}

/* 256-bit values: a field element, a scalar, or raw bytes as a number */
struct fdt_u256 { uint32_t v[8]; };

FDT_HD bool fdt_u256_is_zero(const fdt_u256 &a) {
  uint32_t o = 0;
  FDT_UNROLL
  for (int i = 0; i < 8; i++) o |= a.v[i];
  return o == 0;
}
FDT_HD bool fdt_u256_eq(const fdt_u256 &a, const fdt_u256 &b) {
  uint32_t o = 0;
  FDT_UNROLL
  for (int i = 0; i < 8; i++) o |= a.v[i] ^ b.v[i];
  return o == 0;
}
/* a >= b */
FDT_HD bool fdt_u256_ge(const fdt_u256 &a, const uint32_t *b) {
  uint64_t bw = 0;
  FDT_UNROLL
  for (int i = 0; i < 8; i++) bw = ((uint64_t)a.v[i] - b[i] - bw) >> 63;
  return bw == 0;
}
FDT_HD void fdt_u256_set(fdt_u256 &r, uint32_t w) {
  r.v[0] = w;
  FDT_UNROLL
  for (int i = 1; i < 8; i++) r.v[i] = 0;
}
/* r = c ? a : b */
FDT_HD void fdt_u256_sel(fdt_u256 &r, bool c, const fdt_u256 &a, const fdt_u256 &b) {
  FDT_UNROLL
  for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
}
/* r = (a + b) mod m for a, b < m = 2^256 - c: the sum is >= m when it carries out of 2^256 or when sum + c does */
template <int K>
FDT_HD void fdt_mp_addmod(fdt_u256 &r, const fdt_u256 &a, const fdt_u256 &b, const uint32_t *c) {
  uint32_t s[8], u[8];
  uint64_t c1 = 0, c2 = 0;
  FDT_UNROLL
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)a.v[i] + b.v[i] + c1;
    s[i] = (uint32_t)t;
    c1 = t >> 32;
    const uint64_t w = (uint64_t)s[i] + (i < K ? c[i] : 0u) + c2;
    u[i] = (uint32_t)w;
    c2 = w >> 32;
  }
  const bool over = (c1 | c2) != 0;
  FDT_UNROLL
  for (int i = 0; i < 8; i++) r.v[i] = over ? u[i] : s[i];
}
/* r = (a - b) mod m for a, b < m = 2^256 - c: a borrow is made good by + m, which is - c mod 2^256 */
template <int K>
FDT_HD void fdt_mp_submod(fdt_u256 &r, const fdt_u256 &a, const fdt_u256 &b, const uint32_t *c) {
  uint32_t d[8], u[8];
  uint64_t b1 = 0, b2 = 0;
  FDT_UNROLL
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)a.v[i] - b.v[i] - b1;
    d[i] = (uint32_t)t;
    b1 = t >> 63;
    const uint64_t w = (uint64_t)d[i] - (i < K ? c[i] : 0u) - b2;
    u[i] = (uint32_t)w;
    b2 = w >> 63;
  }
  FDT_UNROLL
  for (int i = 0; i < 8; i++) r.v[i] = b1 ? u[i] : d[i];
}

/* ------------------------------------------------------- the field mod p */

#define FDT_K1_PC {0x000003d1u, 0x00000001u}                               /* 2^256 - p = 2^32 + 977 */
#define FDT_K1_P {0xfffffc2fu, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}

/* a, b any 256-bit values (not only reduced ones); r < p */
FDT_HD void fdt_fe_mul(fdt_u256 &r, const fdt_u256 &a, const fdt_u256 &b) {
  constexpr uint32_t pc[2] = FDT_K1_PC;
  uint32_t t[16];
  fdt_mp_mul<8, 8>(a.v, b.v, t);
  fdt_mp_reduce<2>(t, pc, r.v);
}
FDT_HD void fdt_fe_sqr(fdt_u256 &r, const fdt_u256 &a) { fdt_fe_mul(r, a, a); }
/* a, b < p */
FDT_HD void fdt_fe_add(fdt_u256 &r, const fdt_u256 &a, const fdt_u256 &b) {
  constexpr uint32_t pc[2] = FDT_K1_PC;
  fdt_mp_addmod<2>(r, a, b, pc);
}
FDT_HD void fdt_fe_sub(fdt_u256 &r, const fdt_u256 &a, const fdt_u256 &b) {
  constexpr uint32_t pc[2] = FDT_K1_PC;
  fdt_mp_submod<2>(r, a, b, pc);
}
/* r = a^e, e a public 256-bit exponent: 256 squarings and a product per set bit */
FDT_HD void fdt_fe_pow(fdt_u256 &r, const fdt_u256 &a, const uint32_t *e) {
  fdt_u256 acc;
  fdt_u256_set(acc, 1u);
  FDT_NOUNROLL
  for (int i = 255; i >= 0; i--) {
    fdt_fe_sqr(acc, acc);
    if ((e[i >> 5] >> (i & 31)) & 1u) fdt_fe_mul(acc, acc, a);
  }
  r = acc;
}
/* r = a^(p-2): 1 / a, and 0 for a = 0 */
FDT_HD void fdt_fe_inv(fdt_u256 &r, const fdt_u256 &a) {
  constexpr uint32_t e[8] = {0xfffffc2du, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  fdt_fe_pow(r, a, e);
}
/* p = 3 (mod 4): r = a^((p+1)/4) is a square root of a when a has one.  Returns whether r^2 = a. */
FDT_HD bool fdt_fe_sqrt(fdt_u256 &r, const fdt_u256 &a) {
  constexpr uint32_t e[8] = {0xbfffff0cu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x3fffffffu};
  fdt_u256 one, ar, q;
  fdt_u256_set(one, 1u);
  fdt_fe_mul(ar, a, one);                       /* a reduced */
  fdt_fe_pow(r, ar, e);
  fdt_fe_sqr(q, r);
  return fdt_u256_eq(q, ar);
}

/* ---------------------------------------------------- scalars mod n */

#define FDT_K1_NC {0x2fc9bebfu, 0x402da173u, 0x50b75fc4u, 0x45512319u, 0x00000001u}   /* 2^256 - n */
#define FDT_K1_N {0xd0364141u, 0xbfd25e8cu, 0xaf48a03bu, 0xbaaedce6u, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu}

FDT_HD void fdt_sc_mul(fdt_u256 &r, const fdt_u256 &a, const fdt_u256 &b) {
  constexpr uint32_t nc[5] = FDT_K1_NC;
  uint32_t t[16];
  fdt_mp_mul<8, 8>(a.v, b.v, t);
  fdt_mp_reduce<5>(t, nc, r.v);
}
/* a any 256-bit value: a < 2^256 < 2 n, one conditional subtraction */
FDT_HD void fdt_sc_reduce(fdt_u256 &r, const fdt_u256 &a) {
  constexpr uint32_t nc[5] = FDT_K1_NC;
  uint32_t u[8];
  uint64_t cy = 0;
  FDT_UNROLL
  for (int i = 0; i < 8; i++) {
    const uint64_t s = (uint64_t)a.v[i] + (i < 5 ? nc[i] : 0u) + cy;
    u[i] = (uint32_t)s;
    cy = s >> 32;
  }
  FDT_UNROLL
  for (int i = 0; i < 8; i++) r.v[i] = cy ? u[i] : a.v[i];
}
/* a < n */
FDT_HD void fdt_sc_neg(fdt_u256 &r, const fdt_u256 &a) {
  constexpr uint32_t nc[5] = FDT_K1_NC;
  fdt_u256 z;
  fdt_u256_set(z, 0u);
  fdt_mp_submod<5>(r, z, a, nc);
}
/* r = a^(n-2): 1 / a mod n, and 0 for a = 0 */
FDT_HD void fdt_sc_inv(fdt_u256 &r, const fdt_u256 &a) {
  constexpr uint32_t e[8] = {0xd036413fu, 0xbfd25e8cu, 0xaf48a03bu, 0xbaaedce6u, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  fdt_u256 acc;
  fdt_u256_set(acc, 1u);
  FDT_NOUNROLL
  for (int i = 255; i >= 0; i--) {
    fdt_sc_mul(acc, acc, acc);
    if ((e[i >> 5] >> (i & 31)) & 1u) fdt_sc_mul(acc, acc, a);
  }
  r = acc;
}

/* ------------------------------------------------------------- the group */

/* y^2 = x^3 + 7 in Jacobian coordinates; z = 0: the point at infinity */
struct fdt_k1_point { fdt_u256 x, y, z; };

FDT_HD void fdt_k1_set_infinity(fdt_k1_point &r) {
  fdt_u256_set(r.x, 1u); fdt_u256_set(r.y, 1u); fdt_u256_set(r.z, 0u);
}
FDT_HD bool fdt_k1_is_infinity(const fdt_k1_point &a) { return fdt_u256_is_zero(a.z); }

/* r = 2 a (dbl-2009-l for a curve with a = 0: 2 products, 5 squarings).  Infinity doubles to infinity: z3 = 2 y z. */
FDT_HD void fdt_k1_dbl(fdt_k1_point &r, const fdt_k1_point &p) {
  fdt_u256 a, b, c, d, e, f, t;
  fdt_fe_sqr(a, p.x);
  fdt_fe_sqr(b, p.y);
  fdt_fe_sqr(c, b);
  fdt_fe_add(t, p.x, b);
  fdt_fe_sqr(t, t);
  fdt_fe_sub(t, t, a);
  fdt_fe_sub(t, t, c);
  fdt_fe_add(d, t, t);                          /* d = 2 ((x + b)^2 - a - c) = 4 x y^2 */
  fdt_fe_add(e, a, a);
  fdt_fe_add(e, e, a);                          /* e = 3 x^2 */
  fdt_fe_sqr(f, e);
  fdt_fe_mul(t, p.y, p.z);
  fdt_fe_add(r.z, t, t);                        /* z3 = 2 y z */
  fdt_fe_sub(f, f, d);
  fdt_fe_sub(r.x, f, d);                        /* x3 = e^2 - 2 d */
  fdt_fe_sub(t, d, r.x);
  fdt_fe_mul(t, e, t);
  fdt_fe_add(c, c, c);
  fdt_fe_add(c, c, c);
  fdt_fe_add(c, c, c);
  fdt_fe_sub(r.y, t, c);                        /* y3 = e (d - x3) - 8 y^4 */
}

/* r = a + b, any a and b (r may be a or b).  With u = x z'^2 and s = y z'^3 of
   each operand over the other's z: the points have the same x when u1 = u2;
   then they are equal (s1 = s2: the sum is the double) or opposite (the sum
   is infinity).  Otherwise the chord: h = u2 - u1, w = s2 - s1, x3 = w^2 -
   h^3 - 2 u1 h^2, y3 = w (u1 h^2 - x3) - s1 h^3, z3 = z1 z2 h. */
FDT_HD void fdt_k1_add(fdt_k1_point &r, const fdt_k1_point &a, const fdt_k1_point &b) {
  if (fdt_k1_is_infinity(a)) { r = b; return; }
  if (fdt_k1_is_infinity(b)) { r = a; return; }
  fdt_u256 z1z1, z2z2, u1, u2, s1, s2, h, w, t;
  fdt_fe_sqr(z1z1, a.z);
  fdt_fe_sqr(z2z2, b.z);
  fdt_fe_mul(u1, a.x, z2z2);
  fdt_fe_mul(u2, b.x, z1z1);
  fdt_fe_mul(t, b.z, z2z2);
  fdt_fe_mul(s1, a.y, t);
  fdt_fe_mul(t, a.z, z1z1);
  fdt_fe_mul(s2, b.y, t);
  fdt_fe_sub(h, u2, u1);
  fdt_fe_sub(w, s2, s1);
  if (fdt_u256_is_zero(h)) {
    if (fdt_u256_is_zero(w)) fdt_k1_dbl(r, a);
    else fdt_k1_set_infinity(r);
    return;
  }
  fdt_u256 h2, h3, v, x3, y3, z3;
  fdt_fe_sqr(h2, h);
  fdt_fe_mul(h3, h, h2);
  fdt_fe_mul(v, u1, h2);
  fdt_fe_sqr(x3, w);
  fdt_fe_sub(x3, x3, h3);
  fdt_fe_sub(x3, x3, v);
  fdt_fe_sub(x3, x3, v);
  fdt_fe_sub(t, v, x3);
  fdt_fe_mul(y3, w, t);
  fdt_fe_mul(t, s1, h3);
  fdt_fe_sub(y3, y3, t);
  fdt_fe_mul(t, a.z, b.z);
  fdt_fe_mul(z3, t, h);
  r.x = x3; r.y = y3; r.z = z3;
}

/* a, not infinity, to affine (x, y) */
FDT_HD void fdt_k1_affine(fdt_u256 &x, fdt_u256 &y, const fdt_k1_point &a) {
  fdt_u256 zi, zi2;
  fdt_fe_inv(zi, a.z);
  fdt_fe_sqr(zi2, zi);
  fdt_fe_mul(x, a.x, zi2);
  fdt_fe_mul(zi2, zi2, zi);
  fdt_fe_mul(y, a.y, zi2);
}

/* r = u1 G + u2 b for an affine b = (bx, by) on the curve and u1, u2 < n:
   256 steps over the two scalars' bits together, each a doubling and, where
   either bit is set, one addition of G, b or G + b.  The additions meet
   infinity (the start, and G + b for b = -G), equal points (b = G, or the
   running sum equal to the table point) and opposite points; fdt_k1_add
   takes them all. */
FDT_HD void fdt_k1_mul2(fdt_k1_point &r, const fdt_u256 &u1, const fdt_u256 &u2, const fdt_u256 &bx, const fdt_u256 &by) {
  constexpr uint32_t gx[8] = {0x16f81798u, 0x59f2815bu, 0x2dce28d9u, 0x029bfcdbu, 0xce870b07u, 0x55a06295u, 0xf9dcbbacu, 0x79be667eu};
  constexpr uint32_t gy[8] = {0xfb10d4b8u, 0x9c47d08fu, 0xa6855419u, 0xfd17b448u, 0x0e1108a8u, 0x5da4fbfcu, 0x26a3c465u, 0x483ada77u};
  fdt_k1_point g, b, gb, q;
  FDT_UNROLL
  for (int i = 0; i < 8; i++) { g.x.v[i] = gx[i]; g.y.v[i] = gy[i]; }
  fdt_u256_set(g.z, 1u);
  b.x = bx; b.y = by;
  fdt_u256_set(b.z, 1u);
  fdt_k1_add(gb, g, b);
  fdt_k1_set_infinity(q);
  FDT_NOUNROLL
  for (int i = 255; i >= 0; i--) {
    fdt_k1_dbl(q, q);
    const uint32_t k = ((u1.v[i >> 5] >> (i & 31)) & 1u) | (((u2.v[i >> 5] >> (i & 31)) & 1u) << 1);
    if (k) {
      fdt_k1_point t;
      fdt_u256_sel(t.x, k == 3u, gb.x, b.x); fdt_u256_sel(t.x, k == 1u, g.x, t.x);
      fdt_u256_sel(t.y, k == 3u, gb.y, b.y); fdt_u256_sel(t.y, k == 1u, g.y, t.y);
      fdt_u256_sel(t.z, k == 3u, gb.z, g.z);                  /* G and b share z = 1 */
      fdt_k1_add(q, q, t);
    }
  }
  r = q;
}

/* ----------------------------------------------------------- the recover */

/* a record's codes; 0 passes.  The names are include/fd_secp256k1_gpu.h's. */
#define FDT_SECP256K1_ERR_RECID    FDGPU_SECP256K1_ERR_RECID
#define FDT_SECP256K1_ERR_RANGE    FDGPU_SECP256K1_ERR_RANGE
#define FDT_SECP256K1_ERR_POINT    FDGPU_SECP256K1_ERR_POINT
#define FDT_SECP256K1_ERR_INFINITY FDGPU_SECP256K1_ERR_INFINITY
#define FDT_SECP256K1_ERR_ADDRESS  FDGPU_SECP256K1_ERR_ADDRESS

/* The public key (x, y) of the signature (r, s, recid) over the 32-byte hash
   h, all as numbers; 0 or the code.  libsecp256k1 v0.5.0's rules:
     recid outside 0..3 fails        secp256k1_ecdsa_recoverable_signature_parse_compact's ARG_CHECK, made a
                                     plain failure by fd_secp256k1_recover (fd_secp256k1.c:19)
     r >= n or s >= n fails          parse_compact: secp256k1_scalar_set_b32 reports overflow
     r = 0 or s = 0 fails            secp256k1_ecdsa_sig_recover
     recid & 2: x = r + n, failing where r >= p - n; else x = r
     y^2 = x^3 + 7 must be a square  secp256k1_ge_set_xo_var; y takes the parity recid & 1
     m = h mod n                     secp256k1_scalar_set_b32, overflow ignored
     Q = (s / r) R - (m / r) G, failing at infinity; a high s passes */
FDT_HD int fdt_secp256k1_recover_core(const fdt_u256 &h, const fdt_u256 &r, const fdt_u256 &s, uint32_t recid, fdt_u256 &qx,
                                      fdt_u256 &qy) {
  constexpr uint32_t n[8] = FDT_K1_N;
  constexpr uint32_t p_minus_n[8] = {0x2fc9baeeu, 0x402da172u, 0x50b75fc4u, 0x45512319u, 0x00000001u, 0u, 0u, 0u};
  fdt_u256_set(qx, 0u);
  fdt_u256_set(qy, 0u);
  if (recid > 3u) return FDT_SECP256K1_ERR_RECID;
  if (fdt_u256_ge(r, n) || fdt_u256_ge(s, n) || fdt_u256_is_zero(r) || fdt_u256_is_zero(s)) return FDT_SECP256K1_ERR_RANGE;
  fdt_u256 x = r;
  if (recid & 2u) {
    if (fdt_u256_ge(r, p_minus_n)) return FDT_SECP256K1_ERR_POINT;
    uint64_t cy = 0;                              /* r + n = r - (2^256 - n) + 2^256 < p */
    FDT_UNROLL
    for (int i = 0; i < 8; i++) {
      const uint64_t t = (uint64_t)r.v[i] + n[i] + cy;
      x.v[i] = (uint32_t)t;
      cy = t >> 32;
    }
  }
  fdt_u256 y2, y, seven, t;
  fdt_u256_set(seven, 7u);
  fdt_fe_sqr(t, x);
  fdt_fe_mul(t, t, x);
  fdt_fe_add(y2, t, seven);
  if (!fdt_fe_sqrt(y, y2)) return FDT_SECP256K1_ERR_POINT;
  if ((y.v[0] & 1u) != (recid & 1u)) {
    fdt_u256 z;
    fdt_u256_set(z, 0u);
    fdt_fe_sub(y, z, y);
  }
  fdt_u256 m, ri, u1, u2;
  fdt_sc_reduce(m, h);
  fdt_sc_inv(ri, r);
  fdt_sc_mul(u1, m, ri);
  fdt_sc_neg(u1, u1);
  fdt_sc_mul(u2, s, ri);
  fdt_k1_point q;
  fdt_k1_mul2(q, u1, u2, x, y);
  if (fdt_k1_is_infinity(q)) return FDT_SECP256K1_ERR_INFINITY;
  fdt_k1_affine(qx, qy, q);
  return 0;
}

/* 32 big-endian bytes at r.at(off ...) as a number */
template <class Reader>
FDT_HD void fdt_u256_load_be(fdt_u256 &a, Reader &r, uint64_t off) {
  FDT_UNROLL
  for (int i = 0; i < 8; i++) {
    const uint64_t k = off + 4u * (7 - i);
    a.v[i] = (r.at(k) << 24) | (r.at(k + 1u) << 16) | (r.at(k + 2u) << 8) | r.at(k + 3u);
  }
}
FDT_HD uint32_t fdt_bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

/* keccak256(x || y), both 32 big-endian bytes: one block */
FDT_HD void fdt_secp256k1_key_hash(uint64_t st[25], const fdt_u256 &x, const fdt_u256 &y) {
  fdt_keccak256_init(st);
  FDT_UNROLL
  for (int k = 0; k < 4; k++) {
    st[k] = (uint64_t)fdt_bswap32(x.v[7 - 2 * k]) | ((uint64_t)fdt_bswap32(x.v[6 - 2 * k]) << 32);
    st[4 + k] = (uint64_t)fdt_bswap32(y.v[7 - 2 * k]) | ((uint64_t)fdt_bswap32(y.v[6 - 2 * k]) << 32);
  }
  st[8] = 0x01ull;
  st[16] = 0x80ull << 56;
  fdt_keccak_f1600(st);
}

/* the most Keccak blocks a record's message takes: it lies inside a payload
   of at most FDT_TXN_MTU bytes, ceil((1232 + 1) / 136) = 10.  The loop below
   never runs further, whatever a descriptor says. */
#define FDT_SECP256K1_MSG_BLOCKS 10u

/* One record (fd_precompiles.c:289-303): the message r.at(msg_at + [0,
   msg_sz)), the signature's 65 bytes at sig_at, the address' 20 at addr_at;
   0 or the record's code. */
template <class Reader>
FDT_HD int fdt_secp256k1_record_core(Reader &r, uint64_t msg_at, uint32_t msg_sz, uint64_t sig_at, uint64_t addr_at) {
  uint64_t st[25];
  fdt_keccak256_init(st);
  const uint32_t nb0 = fdt_keccak256_block_cnt(msg_sz);
  const uint32_t nb = nb0 < FDT_SECP256K1_MSG_BLOCKS ? nb0 : FDT_SECP256K1_MSG_BLOCKS;
  FDT_NOUNROLL
  for (uint32_t b = 0; b < nb; b++) fdt_keccak256_absorb_block(st, r, msg_at, msg_sz, b);          /* :291 */
  fdt_u256 h, sr, ss, qx, qy;
  FDT_UNROLL
  for (int k = 0; k < 4; k++) {                   /* the digest's bytes, big endian, as a number */
    h.v[7 - 2 * k] = fdt_bswap32((uint32_t)st[k]);
    h.v[6 - 2 * k] = fdt_bswap32((uint32_t)(st[k] >> 32));
  }
  fdt_u256_load_be(sr, r, sig_at);
  fdt_u256_load_be(ss, r, sig_at + 32u);
  const uint32_t recid = r.at(sig_at + 64u);      /* :266 */
  const int rc = fdt_secp256k1_recover_core(h, sr, ss, recid, qx, qy);                               /* :295 */
  if (rc) return rc;
  fdt_secp256k1_key_hash(st, qx, qy);                                                                /* :300 */
  uint32_t diff = 0;
  FDT_UNROLL
  for (uint32_t k = 0; k < 20u; k++) diff |= fdt_keccak256_digest_byte(st, 12u + k) ^ r.at(addr_at + k);   /* :302 */
  return diff ? FDT_SECP256K1_ERR_ADDRESS : 0;
}

/* ------------------------------------------------------------- the walk */

/* KeccakSecp256k11111111111111111111111111111 (fd_solana_keccak_secp_256k_program_id,
   compared at fd_executor.c:263), as little-endian words of its 32 bytes
   04c6fc20 f050ccf0 5584d721 1c9f8cf5 9ec14785 bb166a1e 2830e812 20000000 */
FDT_HD uint32_t fdt_secp256k1_id_word(uint32_t w) {
  return w == 0u ? 0x20fcc604u : w == 1u ? 0xf0cc50f0u : w == 2u ? 0x21d78455u : w == 3u ? 0xf58c9f1cu :
         w == 4u ? 0x8547c19eu : w == 5u ? 0x1e6a16bbu : w == 6u ? 0x12e83028u : 0x00000020u;
}

#define FDT_SECP256K1_DATA_START    12u   /* SECP256K1_DATA_START: 1 + one record (fd_precompiles.c:221) */
#define FDT_SECP256K1_OFFSETS_START  1u   /* SECP256K1_SIGNATURE_OFFSETS_START */
#define FDT_SECP256K1_OFFSETS_SZ    11u   /* SECP256K1_SIGNATURE_OFFSETS_SERIALIZED_SIZE */
#define FDT_SECP256K1_SIG_SZ        65u   /* r | s | recovery id (:259) */
#define FDT_SECP256K1_ADDR_SZ       20u   /* SECP256K1_PUBKEY_SERIALIZED_SIZE: an Ethereum address */

/* The most records a transaction of sz bytes can emit.  The smallest
   transaction with an instruction is 166 bytes (fdt_precompile_sig_bound).
   A secp256k1 instruction with c >= 1 records adds its program index (1), an
   empty account list (1), the data size as a compact-u16, the count byte (1)
   and 11 c of records; the data, 1 + 11 c bytes, has a one-byte size up to
   c = 11 and a two-byte size from c = 12 on.  What a record points to costs
   nothing more, as for Ed25519.  So k >= 1 instructions with R records in
   all take at least 166 + 4 k + 11 R bytes, and one byte more wherever an
   instruction has 12 records or more: R <= 11 fits in 170 + 11 R, and R >=
   12 needs either such an instruction (171 + 11 R) or two instructions
   (174 + 11 R).  That gives (sz - 170) / 11 where that is at most 11, else
   (sz - 171) / 11: 96 at FDT_TXN_MTU. */
FDT_HD uint32_t fdt_secp256k1_sig_bound(uint64_t sz) {
  const uint64_t s = sz < FDT_TXN_MTU ? sz : FDT_TXN_MTU;
  if (s < 170u + FDT_SECP256K1_OFFSETS_SZ) return 0u;
  const uint64_t a = (s - 170u) / FDT_SECP256K1_OFFSETS_SZ;
  return (uint32_t)(a <= 11u ? a : (s - 171u) / FDT_SECP256K1_OFFSETS_SZ);
}

FDT_HD bool fdt_secp256k1_is_program(fdt_precompile_reader &r, const fdt_txn_t *t, const fdt_txn_instr_t &ins) {
  const uint64_t a = (uint64_t)t->acct_addr_off + 32u * ins.program_id;
  FDT_UNROLL
  for (uint32_t w = 0; w < 8u; w++) {
    const uint32_t v = r.at(a + 4u * w) | (r.at(a + 4u * w + 1u) << 8) | (r.at(a + 4u * w + 2u) << 16) |
                       (r.at(a + 4u * w + 3u) << 24);
    if (v != fdt_secp256k1_id_word(w)) return false;
  }
  return true;
}

/* fd_precompile_get_instr_data as this precompile calls it (:255-287): a
   one-byte index.  0, or the error it returns. */
FDT_HD int fdt_secp256k1_resolve(const fdt_txn_t *t, uint32_t idx, uint32_t off, uint32_t size, uint32_t *at) {
  if (idx >= t->instr_cnt) return FDGPU_CODE_PRECOMPILE_DATA_OFFSET;            /* :97-99 */
  if (off + size > t->instr[idx].data_sz) return FDGPU_CODE_PRECOMPILE_SIGNATURE;  /* :106-108; off + size < 2^17 */
  *at = (uint32_t)t->instr[idx].data_off + off;
  return 0;
}

#define FDT_SECP256K1_FAIL_ON_BAD_COUNT 1u   /* the libsecp256k1_fail_on_bad_count feature is active (:230-235) */

/* The walk.  emit(instr_idx, rec_idx, sig_off, addr_off, msg_off, msg_sz)
   (payload offsets) is called for each record that resolves, in order, until
   the first structural failure; out->rec_cnt counts the calls.  out->code is
   0, DATA_SIZE at (instruction, 0xFFFF), or DATA_OFFSET or SIGNATURE at
   (instruction, record); out->ed_instr_cnt counts the secp256k1 instructions
   through the whole transaction, past a failure too. */
template <class Emit>
FDT_HD void fdt_secp256k1_walk_core(const uint8_t *payload, uint64_t payload_sz, const fdt_txn_t *t, uint32_t flags,
                                    Emit &emit, fdt_precompile_walk_t *out) {
  fdt_precompile_reader r;
  r.p = payload;
  (void)payload_sz;
  int32_t code = 0;
  uint32_t f_instr = FDT_PRECOMPILE_NONE, f_rec = FDT_PRECOMPILE_NONE, k1_cnt = 0, rec_cnt = 0;
  const uint32_t instr_cnt = t->instr_cnt <= FDT_TXN_INSTR_MAX ? t->instr_cnt : (uint32_t)FDT_TXN_INSTR_MAX;
  for (uint32_t j = 0; j < instr_cnt; j++) {                 /* fd_executor.c:255 */
    const fdt_txn_instr_t ins = t->instr[j];
    if (!fdt_secp256k1_is_program(r, t, ins)) continue;
    k1_cnt++;
    if (code) continue;                                      /* the reference has returned (fd_executor.c:264-266) */
    const uint32_t data_off = ins.data_off, data_sz = ins.data_sz;
    if (data_sz < FDT_SECP256K1_DATA_START) {                /* :221-226; data[0] is read only when data_sz == 1 */
      if (data_sz == 1u && r.at(data_off) == 0) continue;
      code = FDGPU_CODE_PRECOMPILE_DATA_SIZE; f_instr = j;
      continue;
    }
    const uint32_t cnt = r.at(data_off);                     /* :229 */
    if (cnt == 0u && (flags & FDT_SECP256K1_FAIL_ON_BAD_COUNT)) {   /* :230-235; data_sz >= 12 > 1 here */
      code = FDGPU_CODE_PRECOMPILE_DATA_SIZE; f_instr = j;
      continue;
    }
    if (data_sz < cnt * FDT_SECP256K1_OFFSETS_SZ + FDT_SECP256K1_OFFSETS_START) {   /* :238-241 */
      code = FDGPU_CODE_PRECOMPILE_DATA_SIZE; f_instr = j;
      continue;
    }
    for (uint32_t i = 0; i < cnt; i++) {                     /* :244; cnt <= 255 */
      const uint64_t b = (uint64_t)data_off + FDT_SECP256K1_OFFSETS_START + FDT_SECP256K1_OFFSETS_SZ * i;
      /* fd_secp256k1_signature_offsets_t (fd_precompiles.c:35-43), packed */
      const uint32_t sig_offset = fdt_precompile_u16(r, b), sig_instr = r.at(b + 2u),
                     addr_offset = fdt_precompile_u16(r, b + 3u), addr_instr = r.at(b + 5u),
                     msg_offset = fdt_precompile_u16(r, b + 6u), msg_sz = fdt_precompile_u16(r, b + 8u),
                     msg_instr = r.at(b + 10u);
      uint32_t sig_at = 0, addr_at = 0, msg_at = 0;
      int err = fdt_secp256k1_resolve(t, sig_instr, sig_offset, FDT_SECP256K1_SIG_SZ, &sig_at);        /* :255-261 */
      if (!err) err = fdt_secp256k1_resolve(t, addr_instr, addr_offset, FDT_SECP256K1_ADDR_SZ, &addr_at);   /* :270-276 */
      if (!err) err = fdt_secp256k1_resolve(t, msg_instr, msg_offset, msg_sz, &msg_at);              /* :281-287 */
      if (err) {
        code = err; f_instr = j; f_rec = i;
        break;
      }
      emit(j, i, sig_at, addr_at, msg_at, msg_sz);           /* :291-303: one record's check */
      rec_cnt++;
    }
  }
  out->code = code;
  out->rec_cnt = rec_cnt;
  out->instr_idx = (uint16_t)f_instr;
  out->rec_idx = (uint16_t)f_rec;
  out->ed_instr_cnt = (uint16_t)k1_cnt;
  out->_pad = 0;
}

/* The verdict of a walk whose n = rec_cnt records were all checked:
   fdt_precompile_verdict_core's rule, code_at(k) record k's
   fdt_secp256k1_record_core code.  The first failed record gives SIGNATURE at
   its position with its code kept in info->ed_code; info->ed_instr_cnt is
   the count of secp256k1 instructions. */
template <class CodeAt, class PosAt>
FDT_HD int fdt_secp256k1_verdict_core(int32_t walk_code, uint32_t f_instr, uint32_t f_rec, uint32_t instr_cnt, uint32_t n,
                                      CodeAt code_at, PosAt pos_at, fdgpu_precompile_info_t *info) {
  return fdt_precompile_verdict_core(walk_code, f_instr, f_rec, instr_cnt, n, code_at, pos_at, info);
}
