/* fdgpu_test_kernels.hip -- per-stage diagnostics for the parity tests: each
   kernel runs one stage of the verify (field and scalar arithmetic, point
   decode, SHA-512, k, the lattice split) on given inputs and writes out its
   result.  No batch uses them. */
#include <hip/hip_runtime.h>

#include "fdgpu_atab.h"
#include "fdgpu_ge.h"
#include "fdgpu_hram.h"
#include "fdgpu_internal.h"
#include "fdgpu_lattice.h"
#include "fdgpu_sc.h"
#include "fdgpu_sha512.h"

using namespace fdgpu;

namespace {

/* in: n records of 2 x 8 u32 (a, b < 2^255 as LE words); out: n records of
   8 ops x 8 u32 canonical: a*b, a^2, a+b, a-b, pow22523(a), invert(a), canon(a), -a */
__global__ void __launch_bounds__(64) fdgpu_test_fe_kernel(const uint32_t *in, uint32_t *out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t aw[8], bw[8];
#pragma unroll
  for (int j = 0; j < 8; j++) { aw[j] = in[16 * i + j]; bw[j] = in[16 * i + 8 + j]; }
  fe a, b, r;
  fe_frombytes(a, aw); fe_frombytes(b, bw);
  uint32_t o[8];
  uint32_t *dst = out + 64 * i;
  fe_mul(r, a, b); fe_tobytes(o, r);
  for (int j = 0; j < 8; j++) dst[j] = o[j];
  fe_sq(r, a); fe_tobytes(o, r);
  for (int j = 0; j < 8; j++) dst[8 + j] = o[j];
  fe_add(r, a, b); fe_tobytes(o, r);
  for (int j = 0; j < 8; j++) dst[16 + j] = o[j];
  fe_sub(r, a, b); fe_tobytes(o, r);
  for (int j = 0; j < 8; j++) dst[24 + j] = o[j];
  fe_pow22523(r, a); fe_tobytes(o, r);
  for (int j = 0; j < 8; j++) dst[32 + j] = o[j];
  fe_invert(r, a); fe_tobytes(o, r);
  for (int j = 0; j < 8; j++) dst[40 + j] = o[j];
  fe_tobytes(o, a);
  for (int j = 0; j < 8; j++) dst[48 + j] = o[j];
  fe_neg(r, a); fe_tobytes(o, r);
  for (int j = 0; j < 8; j++) dst[56 + j] = o[j];
}

/* in: n encodings (8 u32); out: n x 18 u32: [rc, small_order, x(8), y(8)] */
__global__ void __launch_bounds__(64) fdgpu_test_decode_kernel(const uint32_t *enc, uint32_t *out, uint32_t n, uint32_t flags) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t e[8];
  for (int j = 0; j < 8; j++) e[j] = enc[8 * i + j];
  ge_p3 P;
  const bool ok = ge_decode(P, e, (flags & FDGPU_FLAG_REF_MAP) != 0);
  uint32_t *dst = out + 18 * i;
  dst[0] = ok ? 0u : 0xffffffffu;
  dst[1] = ok ? (ge_is_small_order_affine(P) ? 1u : 0u) : 0xffffffffu;
  uint32_t x[8], y[8];
  fe_tobytes(x, P.X); fe_tobytes(y, P.Y);
  for (int j = 0; j < 8; j++) { dst[2 + j] = x[j]; dst[10 + j] = y[j]; }
}

/* SHA-512 of arena[msg_off .. +msg_sz]; out: n x 16 u32 (digest bytes, LE words) */
__global__ void __launch_bounds__(64) fdgpu_test_sha512_kernel(const uint8_t *arena, const fdgpu_sig_desc_t *msgs, uint32_t n,
                                         uint32_t *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  const fdgpu_sig_desc_t d = msgs[active ? i : n - 1];
  uint32_t nb = (d.msg_sz + 16u) / 128u + 1u;
  for (int off = 32; off > 0; off >>= 1) nb = max(nb, (uint32_t)__shfl_xor((int)nb, off));
  uint64_t h[8];
  sha512_plain(h, arena + d.msg_off, d.msg_sz, nb);
  if (!active) return;
  for (int j = 0; j < 8; j++) {
    out[16 * i + 2 * j] = bswap32((uint32_t)(h[j] >> 32));
    out[16 * i + 2 * j + 1] = bswap32((uint32_t)h[j]);
  }
}

/* k = SHA-512(R||A||M) mod L per signature; out: n x 8 u32 */
__global__ void __launch_bounds__(64) fdgpu_test_hram_kernel(const uint8_t *arena, const fdgpu_sig_desc_t *sigs, uint32_t n,
                                       uint32_t *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = i < n;
  const fdgpu_sig_desc_t d = sigs[active ? i : n - 1];
  const uint32_t nb = wave_max_u32(sha512_hram_blocks(d.msg_sz));
  uint32_t R[8], A[8], k[8];
  load32(R, arena + d.sig_off);
  load32(A, arena + d.pub_off);
  hram_k(k, R, A, arena, d, nb);
  if (!active) return;
  for (int j = 0; j < 8; j++) out[8 * i + j] = k[j];
}

__global__ void __launch_bounds__(64) fdgpu_test_sc_reduce_kernel(const uint32_t *in, uint32_t *out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t x[16], r[8];
  for (int j = 0; j < 16; j++) x[j] = in[16 * i + j];
  sc_reduce512(r, x);
  for (int j = 0; j < 8; j++) out[8 * i + j] = r[j];
}

/* hs_split on the device (v_rcp_f64 quotients) for the parity tests: n
   scalars k < L (8 words each) -> 16 words each: |u| (5), |v| (5), ok,
   u_neg, v_neg, bits, 0, 0 */
__global__ void __launch_bounds__(64) fdgpu_test_hs_split_kernel(const uint32_t *in, uint32_t *out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t k[8];
  for (int j = 0; j < 8; j++) k[j] = i < n ? in[8 * i + j] : 0u;
  hs_split_t o;
  hs_split(o, k);                               /* every lane runs it: the loops are wave-uniform */
  if (i >= n) return;
  uint32_t *w = out + 16 * (size_t)i;
  for (int j = 0; j < 5; j++) { w[j] = o.u[j]; w[5 + j] = o.v[j]; }
  w[10] = o.ok; w[11] = o.u_neg; w[12] = o.v_neg; w[13] = o.bits; w[14] = 0u; w[15] = 0u;
}

FDG_DEV void put_fe(uint32_t *dst, const fe &f) {
  uint32_t o[8];
  fe_tobytes(o, f);
#pragma unroll
  for (int j = 0; j < 8; j++) dst[j] = o[j];
}

/* Field ops on raw limb vectors (no fe_frombytes: the limbs are taken as they
   are, so the test picks them at the bounds of the classes R, A, S, S4 of
   fdgpu_fe.h).  in: n records of 2 x 10 u32 (f, g); out: n records of 10 x 8
   u32 canonical: f*g, f^2, f+g, f-g, (f-g)*g, -f, (-f)*g, canon(f), f-g by 4p,
   (f-g by 4p)*g.  An op whose precondition the record does not meet computes
   garbage (plain 32-bit arithmetic, nothing else); the test compares only the
   ops each record is inside the contract of. */
__global__ void __launch_bounds__(64) fdgpu_test_fe_raw_kernel(const uint32_t *in, uint32_t *out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fe f, g, r, s;
#pragma unroll
  for (int j = 0; j < 10; j++) { f.v[j] = in[20 * (size_t)i + j]; g.v[j] = in[20 * (size_t)i + 10 + j]; }
  uint32_t *dst = out + 80 * (size_t)i;
  fe_mul(r, f, g);  put_fe(dst, r);
  fe_sq(r, f);      put_fe(dst + 8, r);
  fe_add(r, f, g);  put_fe(dst + 16, r);
  fe_sub(s, f, g);  put_fe(dst + 24, s);
  fe_mul(r, s, g);  put_fe(dst + 32, r);
  fe_neg(s, f);     put_fe(dst + 40, s);
  fe_mul(r, s, g);  put_fe(dst + 48, r);
  put_fe(dst + 56, f);
  fe_sub4(s, f, g); put_fe(dst + 64, s);
  fe_mul(r, s, g);  put_fe(dst + 72, r);
}

FDG_DEV void get_fe(fe &h, const uint32_t *src) {
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = src[j];
  fe_frombytes(h, w);
}
FDG_DEV void put_p3(uint32_t *dst, const ge_p3 &p) {
  put_fe(dst, p.X); put_fe(dst + 8, p.Y); put_fe(dst + 16, p.Z); put_fe(dst + 24, p.T);
}
FDG_DEV void put_p2(uint32_t *dst, const ge_p2 &p) {
  put_fe(dst, p.X); put_fe(dst + 8, p.Y); put_fe(dst + 16, p.Z);
#pragma unroll
  for (int j = 0; j < 8; j++) dst[24 + j] = 0u;
}
FDG_DEV void put_p1p1(uint32_t *dst, const ge_p1p1 &t) {
  ge_p3 r;
  ge_p1p1_to_p3(r, t);
  put_p3(dst, r);
}

/* words per record of the group-op kernel: P, Q (X, Y, Z, T: 8 LE words each)
   and Q's affine niels form (y+x, y-x, 2dxy: canonical, 8 words each) in;
   GE_RESULTS points (X, Y, Z, T canonical; T = 0 for a p2 result) out */
#define GE_IN_WORDS  88u
#define GE_RESULTS   21u
#define GE_OUT_WORDS (GE_RESULTS * 32u)

/* Every group operation of fdgpu_ge.h on one pair (P, Q), one lane per
   record.  Results, in order (a pair = neg false, then neg true):
     0      ge_dbl(P) through ge_p1p1_to_p3           1   through ge_p1p1_to_p2
     2,3    ge_add_cached(P, ge_p3_to_cached(Q))      4,5   ge_add_cached_ld over that entry
     6,7    ge_add_cached_regs (entry flattened)      8,9   ge_add_cached_regs_swapped (Y+X / Y-X
                                                            handed over as unstage_entry_signed does)
     10,11  ge_add_niels                              12,13 ge_add_niels_regs
     14,15  ge_cached_regs_to_p2                      16,17 ge_niels_regs_to_p3
     18     ge_p3_neg(P)
     19,20  one chain window: four (ge_dbl, ge_p1p1_to_p2), T = t.X t.Y, then + Q and +- Q by
            ge_add_cached_regs_swapped: 16P + 2Q, 16P */
__global__ void __launch_bounds__(64) fdgpu_test_ge_kernel(const uint32_t *in, uint32_t *out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t *src = in + GE_IN_WORDS * (size_t)i;
  uint32_t *dst = out + GE_OUT_WORDS * (size_t)i;
  ge_p3 P, Q;
  get_fe(P.X, src); get_fe(P.Y, src + 8); get_fe(P.Z, src + 16); get_fe(P.T, src + 24);
  get_fe(Q.X, src + 32); get_fe(Q.Y, src + 40); get_fe(Q.Z, src + 48); get_fe(Q.T, src + 56);
  ge_niels N;
  get_fe(N.ypx, src + 64); get_fe(N.ymx, src + 72); get_fe(N.xy2d, src + 80);
  ge_cached C;
  ge_p3_to_cached(C, Q);
  uint32_t qc[40], qn[32];
#pragma unroll
  for (int w = 0; w < 10; w++) {
    qc[w] = C.YpX.v[w]; qc[10 + w] = C.YmX.v[w]; qc[20 + w] = C.Z2.v[w]; qc[30 + w] = C.T2d.v[w];
    qn[w] = N.ypx.v[w]; qn[10 + w] = N.ymx.v[w]; qn[20 + w] = N.xy2d.v[w];
  }
  qn[30] = 0u; qn[31] = 0u;

  ge_p1p1 t;
  ge_p2 a2;
  ge_p3 r3;
  ge_p3_to_p2(a2, P);
  ge_dbl(t, a2);
  put_p1p1(dst, t);
  ge_p1p1_to_p2(a2, t);
  put_p2(dst + 32, a2);

  auto ldc = [&C](int c, int w) { return c == 0 ? C.YpX.v[w] : c == 1 ? C.YmX.v[w] : c == 2 ? C.Z2.v[w] : C.T2d.v[w]; };
#pragma unroll 1
  for (int s = 0; s < 2; s++) {
    const bool neg = s != 0;
    uint32_t *d = dst + 32 * s;
    ge_add_cached(t, P, C, neg);          put_p1p1(d + 32 * 2, t);
    ge_add_cached_ld(t, P, ldc, neg);     put_p1p1(d + 32 * 4, t);
    ge_add_cached_regs(t, P, qc, neg);    put_p1p1(d + 32 * 6, t);
    uint32_t qs[40];
#pragma unroll
    for (int w = 0; w < 10; w++) {
      qs[w] = neg ? qc[10 + w] : qc[w]; qs[10 + w] = neg ? qc[w] : qc[10 + w]; qs[20 + w] = qc[20 + w]; qs[30 + w] = qc[30 + w];
    }
    ge_add_cached_regs_swapped(t, P, qs, neg); put_p1p1(d + 32 * 8, t);
    ge_add_niels(t, P, N, neg);           put_p1p1(d + 32 * 10, t);
    ge_add_niels_regs(t, P, qn, neg);     put_p1p1(d + 32 * 12, t);
    ge_cached_regs_to_p2(a2, qc, neg);    put_p2(d + 32 * 14, a2);
    ge_niels_regs_to_p3(r3, qn, neg);     put_p3(d + 32 * 16, r3);

    /* the window as hs_chain performs it */
    ge_p3_to_p2(a2, P);
#pragma unroll 1
    for (int k = 0; k < 4; k++) { ge_dbl(t, a2); ge_p1p1_to_p2(a2, t); }
    r3.X = a2.X; r3.Y = a2.Y; r3.Z = a2.Z; fe_mul(r3.T, t.X, t.Y);
    ge_add_cached_regs_swapped(t, r3, qc, false);
    ge_p1p1_to_p3(r3, t);
    ge_add_cached_regs_swapped(t, r3, qs, neg);
    put_p1p1(d + 32 * 19, t);
  }
  ge_p3_neg(r3, P);
  put_p3(dst + 32 * 18, r3);
}

/* in: n scalars (8 words); out: n x 16 words: sc_recode16's packed digits (8
   words), then sc_recode_comb<BC_W, BC_NDIG>'s */
__global__ void __launch_bounds__(64) fdgpu_test_sc_recode_kernel(const uint32_t *in, uint32_t *out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int NW = COMB_WORDS(FDGPU_BCOMB_BITS, FDGPU_BCOMB_NDIG);
  static_assert(NW <= 8, "the record holds 8 words of comb digits");
  uint32_t s[8], d16[8], dc[NW];
  for (int j = 0; j < 8; j++) s[j] = in[8 * (size_t)i + j];
  sc_recode16(d16, s);
  sc_recode_comb<(int)FDGPU_BCOMB_BITS, (int)FDGPU_BCOMB_NDIG>(dc, s);
  uint32_t *w = out + 16 * (size_t)i;
  for (int j = 0; j < 8; j++) { w[j] = d16[j]; w[8 + j] = j < NW ? dc[j] : 0u; }
}

/* The packed table entry, one lane per record.  in: the 40 raw limbs of a
   cached entry (Y+X, Y-X, 2Z, 2dT), taken as they are; out, per record
   (FDGPU_TABPACK_OUT_WORDS, a whole number of lines): the 32 words atab_store
   leaves at [0, 32) (as entry 1 of a table whose first stored entry is the
   record's first line), the 40 limbs atab_load returns at [32, 72), those of
   stage_entry + unstage_entry_signed at [72, 112), and of the same with neg
   at [112, 152). */
__global__ void __launch_bounds__(64) fdgpu_test_tabpack_kernel(const uint32_t *in, uint32_t *out, uint32_t n) {
  __shared__ uint32_t s_stage[FDGPU_STAGE_WAVE_WORDS];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t *src = in + FDGPU_ATAB_WORDS * (size_t)i;
  uint32_t *dst = out + FDGPU_TABPACK_OUT_WORDS * (size_t)i;
  ge_cached c;
#pragma unroll
  for (int w = 0; w < 10; w++) { c.YpX.v[w] = src[w]; c.YmX.v[w] = src[10 + w]; c.Z2.v[w] = src[20 + w]; c.T2d.v[w] = src[30 + w]; }
  uint32_t *tab = dst - FDGPU_PTAB_WORDS;       /* virtual base: entry 1 is the record's first line */
  atab_store(tab, 1, c);
  __threadfence();                              /* the entry is read back by this lane, also by LDS-DMA */
  uint32_t q[40];
  atab_load(q, tab, 1);
#pragma unroll
  for (int w = 0; w < 40; w++) dst[32 + w] = q[w];
  stage_entry(s_stage, tab, 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  unstage_entry_signed(q, s_stage, false);
#pragma unroll
  for (int w = 0; w < 40; w++) dst[72 + w] = q[w];
  unstage_entry_signed(q, s_stage, true);
#pragma unroll
  for (int w = 0; w < 40; w++) dst[112 + w] = q[w];
}

}  // namespace

extern "C" {

hipError_t fdgpu_launch_test_fe(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(fdgpu_test_fe_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_in, d_out, n);
  return hipGetLastError();
}
hipError_t fdgpu_launch_test_decode(const uint32_t *d_enc, uint32_t *d_out, uint32_t n, uint32_t flags,
                                    hipStream_t stream) {
  hipLaunchKernelGGL(fdgpu_test_decode_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_enc, d_out, n, flags);
  return hipGetLastError();
}
hipError_t fdgpu_launch_test_sha512(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_msgs, uint32_t n,
                                    uint32_t *d_out, hipStream_t stream) {
  hipLaunchKernelGGL(fdgpu_test_sha512_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_arena, d_msgs, n, d_out);
  return hipGetLastError();
}
hipError_t fdgpu_launch_test_hram(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_sigs, uint32_t n,
                                  uint32_t *d_out, hipStream_t stream) {
  hipLaunchKernelGGL(fdgpu_test_hram_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_arena, d_sigs, n, d_out);
  return hipGetLastError();
}
hipError_t fdgpu_launch_test_sc_reduce(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(fdgpu_test_sc_reduce_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_in, d_out, n);
  return hipGetLastError();
}
hipError_t fdgpu_launch_test_hs_split(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(fdgpu_test_hs_split_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_in, d_out, n);
  return hipGetLastError();
}
hipError_t fdgpu_launch_test_fe_raw(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(fdgpu_test_fe_raw_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_in, d_out, n);
  return hipGetLastError();
}
uint32_t fdgpu_test_ge_in_words(void) { return GE_IN_WORDS; }
uint32_t fdgpu_test_ge_results(void) { return GE_RESULTS; }
hipError_t fdgpu_launch_test_ge(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(fdgpu_test_ge_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_in, d_out, n);
  return hipGetLastError();
}
hipError_t fdgpu_launch_test_sc_recode(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(fdgpu_test_sc_recode_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_in, d_out, n);
  return hipGetLastError();
}
hipError_t fdgpu_launch_test_tabpack(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(fdgpu_test_tabpack_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_in, d_out, n);
  return hipGetLastError();
}

}  // extern "C"
