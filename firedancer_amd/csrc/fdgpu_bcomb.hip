/* fdgpu_bcomb.hip -- builds the fixed-base comb tables (fdgpu_bcomb.h) that
   the verify kernels' [S]B reads: two kernels, run once per device at engine
   open. */
#include <hip/hip_runtime.h>

#include "fdgpu_bcomb.h"
#include "fdgpu_ge.h"
#include "fdgpu_internal.h"

using namespace fdgpu;

namespace {

constexpr uint32_t BC_CHUNKS = (BC_ENT + FDGPU_BCOMB_CHUNK - 1) / FDGPU_BCOMB_CHUNK;

/* bases[i] = 2^(W i) B (p3, 40 words), one lane per table */
__global__ void fdgpu_bcomb_base_kernel(uint32_t *bases) {
  const uint32_t i = threadIdx.x;
  if (i >= BC_NDIG) return;
  constexpr uint32_t BX[10] = FDGPU_FE_BX, BY[10] = FDGPU_FE_BY, BT[10] = FDGPU_FE_BT;
  ge_p3 P; fe_set(P.X, BX); fe_set(P.Y, BY); fe_1(P.Z); fe_set(P.T, BT);
  ge_p1p1 t;
  for (uint32_t n = 0; n < BC_W * i; n++) {
    ge_p2 a; ge_p3_to_p2(a, P); ge_dbl(t, a); ge_p1p1_to_p3(P, t);
  }
  uint32_t *o = bases + 40 * i;
#pragma unroll
  for (int w = 0; w < 10; w++) { o[w] = P.X.v[w]; o[10 + w] = P.Y.v[w]; o[20 + w] = P.Z.v[w]; o[30 + w] = P.T.v[w]; }
}

/* One lane per (table, chunk of 64 entries): j0 * base by double-and-add,
   then 63 consecutive additions, then one inversion for the whole chunk
   (Montgomery's trick over the Z coordinates, prefix products in scratch). */
__global__ void __launch_bounds__(64) fdgpu_bcomb_fill_kernel(const uint32_t *bases, uint32_t *tab,
                                                              uint32_t *scratch) {
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= BC_NDIG * BC_CHUNKS) return;
  const uint32_t ti = lane / BC_CHUNKS, j0 = (lane % BC_CHUNKS) * FDGPU_BCOMB_CHUNK;
  const uint32_t cnt = min(FDGPU_BCOMB_CHUNK, BC_ENT - j0);
  ge_p3 base;
  const uint32_t *b = bases + 40 * ti;
#pragma unroll
  for (int w = 0; w < 10; w++) { base.X.v[w] = b[w]; base.Y.v[w] = b[10 + w]; base.Z.v[w] = b[20 + w]; base.T.v[w] = b[30 + w]; }
  ge_cached bc; ge_p3_to_cached(bc, base);
  ge_p3 P; ge_p3_0(P);
  ge_p1p1 t;
  for (int bit = (int)BC_W - 1; bit >= 0; bit--) {                   /* j0 < 2^(W-1) + 1 */
    ge_p2 a; ge_p3_to_p2(a, P); ge_dbl(t, a); ge_p1p1_to_p3(P, t);
    if ((j0 >> bit) & 1u) { ge_add_cached(t, P, bc, false); ge_p1p1_to_p3(P, t); }
  }
  uint32_t *pre = scratch + (size_t)lane * FDGPU_BCOMB_CHUNK * 10;
  uint32_t *ent0 = tab + ((size_t)ti * BC_ENT + j0) * FDGPU_BCOMB_STRIDE;
  fe acc; fe_1(acc);
  for (uint32_t k = 0; k < cnt; k++) {
    uint32_t *e = ent0 + (size_t)k * FDGPU_BCOMB_STRIDE;
#pragma unroll
    for (int w = 0; w < 10; w++) { e[w] = P.X.v[w]; e[10 + w] = P.Y.v[w]; e[20 + w] = P.Z.v[w]; }
    fe_mul(acc, acc, P.Z);
#pragma unroll
    for (int w = 0; w < 10; w++) pre[10 * k + w] = acc.v[w];
    ge_add_cached(t, P, bc, false); ge_p1p1_to_p3(P, t);
  }
  fe inv; fe_invert(inv, acc);
  constexpr uint32_t D2[10] = FDGPU_FE_D2;
  fe d2; fe_set(d2, D2);
  for (int k = (int)cnt - 1; k >= 0; k--) {
    uint32_t *e = ent0 + (size_t)k * FDGPU_BCOMB_STRIDE;
    fe X, Y, Z, zi;
#pragma unroll
    for (int w = 0; w < 10; w++) { X.v[w] = e[w]; Y.v[w] = e[10 + w]; Z.v[w] = e[20 + w]; }
    if (k > 0) {
      fe pk;
#pragma unroll
      for (int w = 0; w < 10; w++) pk.v[w] = pre[10 * (k - 1) + w];
      fe_mul(zi, inv, pk);
    } else {
      zi = inv;
    }
    fe_mul(inv, inv, Z);
    fe x, y, xy, ypx, ymx, xy2d;
    fe_mul(x, X, zi); fe_mul(y, Y, zi);
    fe_add(ypx, y, x); fe_canon(ypx);
    fe_sub(ymx, y, x); fe_canon(ymx);
    fe_mul(xy, x, y); fe_mul(xy2d, xy, d2); fe_canon(xy2d);
    niels_store(e, ypx, ymx, xy2d);
  }
}

}  // namespace

extern "C" {

size_t fdgpu_btab_bytes(void) { return (size_t)BC_NDIG * BC_ENT * FDGPU_BCOMB_STRIDE * sizeof(uint32_t); }

hipError_t fdgpu_btab_build(uint32_t *d_btab, hipStream_t stream) {
  uint32_t *bases = nullptr, *scratch = nullptr;
  const uint32_t lanes = BC_NDIG * BC_CHUNKS;
  hipError_t e = hipMalloc((void **)&bases, BC_NDIG * 40 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc((void **)&scratch, (size_t)lanes * FDGPU_BCOMB_CHUNK * 10 * sizeof(uint32_t));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fdgpu_bcomb_base_kernel, dim3(1), dim3(64), 0, stream, bases);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(fdgpu_bcomb_fill_kernel, dim3((lanes + 63) / 64), dim3(64), 0, stream, bases, d_btab, scratch);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (bases) (void)hipFree(bases);
  if (scratch) (void)hipFree(scratch);
  return e;
}

}  // extern "C"
