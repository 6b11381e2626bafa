/* fdgpu_test_kernels.hip -- per-stage diagnostics for the parity tests: each
   kernel runs one stage of the verify (field and scalar arithmetic, point
   decode, SHA-512, k, the lattice split) on given inputs and writes out its
   result.  No batch uses them. */
#include <hip/hip_runtime.h>

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

}  // extern "C"
