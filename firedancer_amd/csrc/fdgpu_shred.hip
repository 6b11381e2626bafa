/* fdgpu_shred.hip -- raw Merkle shreds on the device (include/fd_shred_gpu.h):
   the shred tile's checks, the SHA-256 Merkle leaf, the walk up the inclusion
   proof, and the records the verify kernels (fdgpu_verify.hip) take from
   there.

     ingest  one shred per lane: fdt_shred_check (fdt_shred.h, the host
             library's own source), the leaf hash over the ~1.1 KB between the
             signature and the proof, one 66-byte node hash per proof layer,
             the root into the arena's roots region, and the signature
             descriptor of a shred that passed -- a wave's passing lanes take
             consecutive descriptor slots with one atomic add on the batch's
             device-side signature count, as the gathered frag ingest does;
     verify  fdgpu_launch_verify_sigs over those descriptors and that count;
     finish  per shred the single-signature combine (its signature's code),
             or FDGPU_CODE_SHRED_REJECT, and its root next to the codes for
             one read-back.

   A lane's hash is serial work on registers (64 rounds x ~17 blocks for the
   leaf, two blocks per proof layer); lanes of a wave differ only in their
   proof depth, so they diverge little.  One wave per block keeps the slot
   claim to a ballot and one atomic. */
#include <hip/hip_runtime.h>

#include "fdgpu_sha256.h"
#include "fdgpu_shred.h"
#include "fdt_shred.h"

using namespace fdgpu;

namespace {

constexpr sha256_prefix_t LEAF_PREFIX = sha256_prefix_words(FDT_BMTREE_LEAF_PREFIX);
constexpr sha256_prefix_t NODE_PREFIX = sha256_prefix_words(FDT_BMTREE_NODE_PREFIX);

/* fdt_shred_root on the device: the state words h are the root, big-endian */
FDG_DEV void shred_root(uint32_t (&h)[8], const uint8_t *shred, const fdt_shred_chk_t &chk) {
  sha256_msg<true>(h, shred + chk.leaf_off, chk.leaf_end - chk.leaf_off, LEAF_PREFIX);
  for (uint32_t l = 0; l < chk.depth; l++) {
    uint32_t node[5], cur[5], nh[8];
    sha256_load_words<5>(node, shred + chk.proof_off + FDT_SHRED_NODE_SZ * l, 0u);
#pragma unroll
    for (int j = 0; j < 5; j++) cur[j] = h[j];
    const bool cur_left = !((chk.shred_idx >> l) & 1u);
    uint32_t lt[5], rt[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const uint32_t c = cur[j], p = node[j];
      lt[j] = cur_left ? c : p; rt[j] = cur_left ? p : c;
    }
    sha256_node(nh, lt, rt, NODE_PREFIX);
#pragma unroll
    for (int j = 0; j < 8; j++) h[j] = nh[j];
  }
}

__global__ void __launch_bounds__(64) fdgpu_shred_ingest_kernel(uint8_t *arena,
                                                                const fdgpu_shred_t *__restrict__ shreds, uint32_t n,
                                                                uint32_t expected_version, uint32_t roots_off,
                                                                fdgpu_sig_desc_t *__restrict__ sigs,
                                                                fdgpu_txn_desc_t *__restrict__ tds,
                                                                uint32_t *__restrict__ n_sig) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  const bool active = i < n;
  const fdgpu_shred_t sh = shreds[active ? i : n - 1u];
  const uint8_t *shred = arena + sh.off;
  fdt_shred_chk_t chk;
  const bool ok = active && fdt_shred_check_core(shred, sh.sz, (uint16_t)expected_version, &chk);
  if (ok) {
    uint32_t h[8];
    shred_root(h, shred, chk);
    uint4 *dst = (uint4 *)(arena + roots_off + 32ull * i);
    dst[0] = make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]), __builtin_bswap32(h[3]));
    dst[1] = make_uint4(__builtin_bswap32(h[4]), __builtin_bswap32(h[5]), __builtin_bswap32(h[6]), __builtin_bswap32(h[7]));
  }
  /* the wave's passing lanes take consecutive descriptor slots */
  const uint64_t m = __ballot(ok);
  const uint32_t lane = threadIdx.x & 63u, cnt = (uint32_t)__popcll(m);
  uint32_t base = 0;
  if (lane == 0 && cnt) base = atomicAdd(n_sig, cnt);
  base = (uint32_t)__shfl((int)base, 0, 64);
  if (!active) return;
  fdgpu_txn_desc_t td;
  td.sig0 = 0; td.sig_cnt = 0;
  if (ok) {
    const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    fdgpu_sig_desc_t sd;
    sd.msg_off = roots_off + 32u * i;
    sd.msg_sz = 32u;
    sd.sig_off = sh.off;
    sd.pub_off = sh.pub_off;
    sigs[slot] = sd;
    td.sig0 = slot; td.sig_cnt = 1;
  }
  tds[i] = td;
}

__global__ void __launch_bounds__(256) fdgpu_shred_finish_kernel(const fdgpu_txn_desc_t *__restrict__ tds, uint32_t n,
                                                                 const int8_t *__restrict__ sig_codes,
                                                                 const uint8_t *__restrict__ roots,
                                                                 int8_t *__restrict__ codes,
                                                                 uint8_t *__restrict__ roots_out) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const fdgpu_txn_desc_t d = tds[i];
    uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
    int code = FDGPU_CODE_SHRED_REJECT;
    if (d.sig_cnt) {
      code = sig_codes ? sig_codes[d.sig0] : 0;
      const uint4 *src = (const uint4 *)(roots + 32ull * i);
      r0 = src[0]; r1 = src[1];
    }
    codes[i] = (int8_t)code;
    uint4 *dst = (uint4 *)(roots_out + 32ull * i);
    dst[0] = r0; dst[1] = r1;
  }
}

__global__ void __launch_bounds__(64) fdgpu_test_sha256_kernel(const uint8_t *__restrict__ arena,
                                                               const fdgpu_sig_desc_t *__restrict__ msgs, uint32_t n,
                                                               uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const fdgpu_sig_desc_t d = msgs[i];
  uint32_t h[8];
  sha256_msg<false>(h, arena + d.msg_off, d.msg_sz, LEAF_PREFIX);
  for (int j = 0; j < 8; j++) out[8 * i + j] = __builtin_bswap32(h[j]);
}

}  // namespace

extern "C" {

hipError_t fdgpu_launch_shred_ingest(uint8_t *d_arena, const fdgpu_shred_t *d_shreds, uint32_t n,
                                     uint16_t expected_version, uint32_t roots_off, fdgpu_sig_desc_t *d_sigs,
                                     fdgpu_txn_desc_t *d_tds, uint32_t *d_n_sig, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_shred_ingest_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_arena, d_shreds, n,
                     (uint32_t)expected_version, roots_off, d_sigs, d_tds, d_n_sig);
  return hipGetLastError();
}

hipError_t fdgpu_launch_shred_finish(const fdgpu_txn_desc_t *d_tds, uint32_t n, const int8_t *d_sig_codes,
                                     const uint8_t *d_roots, int8_t *d_codes, uint8_t *d_roots_out,
                                     hipStream_t stream) {
  if (!n) return hipSuccess;
  const uint32_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(fdgpu_shred_finish_kernel, dim3(blocks < FDGPU_AUX_BLOCKS ? blocks : FDGPU_AUX_BLOCKS), dim3(256), 0,
                     stream, d_tds, n, d_sig_codes, d_roots, d_codes, d_roots_out);
  return hipGetLastError();
}

hipError_t fdgpu_launch_test_sha256(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_msgs, uint32_t n,
                                    uint32_t *d_out, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_test_sha256_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_arena, d_msgs, n, d_out);
  return hipGetLastError();
}

}  // extern "C"
