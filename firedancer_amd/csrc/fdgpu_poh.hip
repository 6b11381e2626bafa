/* fdgpu_poh.hip -- a block's proof of history on the device
   (include/fd_poh_gpu.h): per entry the chain of hash_cnt SHA-256 over 32
   bytes, the Merkle root of its signatures, the mixin and the comparison with
   the hash the entry claims.

     leaves  one signature per lane across the whole batch: SHA-256(0x00 ||
             sig) into the batch's node buffer (8 big-endian words a node);
     roots   one lane per entry folds its own leaf range layer by layer in
             place -- node j of the next layer is written after nodes 2j and
             2j+1 of this one were read, and j <= 2j, so ascending order is
             safe for a single lane; the root ends in the range's first node.
             Lanes never share nodes: the host rejects a batch whose entries'
             ranges are not ascending and disjoint (fdt_poh_args);
     chains  the hot path.  One chain per lane; a lane runs its chain in
             chunks of FDGPU_POH_CHUNK hashes, and between chunks a lane whose
             chain has ended finishes its entry (mixin, compare, code and
             hash) and takes the next one from the batch's queue.

   The tree is deliberately plain.  A mainnet slot is 64 ticks of 62,500
   hashes, 4,000,000 single-block hashes; a full block's ~2,000 signatures are
   ~2,000 leaves and ~2,000 branches of two blocks each, ~8,000 blocks: 0.2 %
   of the slot's hashing.  A cooperative fold would speed up what is not
   measurable next to the chains.

   The queue is an array of entry indices the host has ordered by hash_cnt,
   longest first (it reads every entry to check it anyway), so the longest
   chains start first and the short ones fill in behind them: a wave's time is
   neither the sum nor the maximum of 64 arbitrary entries.  A wave ballots
   the lanes that need work, one lane adds their count to the queue's head
   (cleared on the stream before the launch), each takes its rank.  A wave
   that has seen the queue empty never asks again, and it leaves when none of
   its lanes has work.  Every loop is bounded by the cap and by n: hash_cnt
   comes from untrusted bytes, an entry above the cap is answered at the head
   of the kernel, is not in the queue, and would be clamped if it were. */
#include <hip/hip_runtime.h>

#include "fdgpu_internal.h"
#include "fdgpu_sha256.h"

using namespace fdgpu;

namespace {

constexpr uint32_t POH_BLOCK = 256;

__global__ void __launch_bounds__(64) fdgpu_poh_leaf_kernel(const uint8_t *__restrict__ arena,
                                                            const uint32_t *__restrict__ sig_offs, uint32_t sig_total,
                                                            uint32_t *__restrict__ nodes) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= sig_total) return;
  uint32_t m[16], h[8];
  sha256_load_words<16>(m, arena + sig_offs[i], 0u);
  sha256_hash65(h, 0u, m);
  uint4 *dst = (uint4 *)(nodes + 8ull * i);
  dst[0] = make_uint4(h[0], h[1], h[2], h[3]);
  dst[1] = make_uint4(h[4], h[5], h[6], h[7]);
}

__global__ void __launch_bounds__(64) fdgpu_poh_root_kernel(const fdgpu_poh_entry_t *__restrict__ entries, uint32_t n,
                                                            uint32_t sig_total, uint32_t *nodes) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t first = entries[i].sig_first;
  uint32_t c = entries[i].sig_cnt;
  if (c > sig_total || first > sig_total - c) return;          /* the host checked it: never out of the buffer */
  uint4 *nd = (uint4 *)(nodes + 8ull * first);
  for (; c > 1u; c = (c + 1u) / 2u)
    for (uint32_t j = 0; j < (c + 1u) / 2u; j++) {
      const uint32_t r = 2u * j + 1u < c ? 2u * j + 1u : c - 1u;
      const uint4 l0 = nd[4u * j], l1 = nd[4u * j + 1u], r0 = nd[2u * r], r1 = nd[2u * r + 1u];
      const uint32_t m[16] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
      uint32_t h[8];
      sha256_hash65(h, 1u, m);
      nd[2u * j] = make_uint4(h[0], h[1], h[2], h[3]);
      nd[2u * j + 1u] = make_uint4(h[4], h[5], h[6], h[7]);
    }
}

FDG_DEV void poh_store(int8_t *codes, uint8_t *hashes, uint32_t i, int code, const uint32_t (&h)[8]) {
  codes[i] = (int8_t)code;
  uint4 *dst = (uint4 *)(hashes + 32ull * i);
  dst[0] = make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]), __builtin_bswap32(h[3]));
  dst[1] = make_uint4(__builtin_bswap32(h[4]), __builtin_bswap32(h[5]), __builtin_bswap32(h[6]), __builtin_bswap32(h[7]));
}

__global__ void __launch_bounds__(POH_BLOCK) fdgpu_poh_chain_kernel(const uint8_t *__restrict__ arena,
                                                                    const fdgpu_poh_entry_t *__restrict__ entries,
                                                                    uint32_t n, const uint32_t *__restrict__ order,
                                                                    uint32_t n_q, const uint32_t *__restrict__ nodes,
                                                                    uint32_t cap, uint32_t n_waves, uint32_t *head,
                                                                    int8_t *__restrict__ codes,
                                                                    uint8_t *__restrict__ hashes) {
  const uint32_t tid = blockIdx.x * POH_BLOCK + threadIdx.x, lane = threadIdx.x & 63u;
  if (tid / 64u >= n_waves) return;                            /* whole waves: tid / 64 is wave-uniform */
  /* entries above the cap: answered here, never started */
  for (uint32_t i = tid; i < n; i += n_waves * 64u)
    if (entries[i].hash_cnt > cap) {
      const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      poh_store(codes, hashes, i, FDGPU_CODE_POH_TOO_LONG, z);
    }
  uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t rem = 0, idx = 0;
  bool have = false, drained = false;                          /* drained is wave-uniform */
  for (;;) {
    const uint64_t need = __ballot(!have);
    if (need && !drained) {
      const uint32_t cnt = (uint32_t)__popcll(need);
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(head, cnt);
      base = (uint32_t)__shfl((int)base, 0, 64);
      const uint32_t my = base + (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
      drained = base >= n_q || n_q - base < cnt;               /* this pull reached the queue's end */
      if (!have && base < n_q && my < n_q) {
        idx = order[my];
        if (idx < n) {
          const fdgpu_poh_entry_t e = entries[idx];
          const bool mixes = e.sig_cnt || e.mix_off != FDGPU_POH_NO_MIX;
          const uint64_t len = mixes ? (e.hash_cnt ? e.hash_cnt - 1u : 0u) : e.hash_cnt;
          if (e.hash_cnt <= cap) {                             /* the queue holds no other; a longer one is not run */
            sha256_load_words<8>(h, arena + e.prev_off, 0u);
            rem = (uint32_t)len;
            have = true;
          }
        }
      }
    }
    if (!__any(have)) break;
#pragma unroll 1
    for (uint32_t k = 0; k < FDGPU_POH_CHUNK; k++)
      if (rem) { sha256_hash32(h); rem--; }
    if (have && !rem) {
      const fdgpu_poh_entry_t e = entries[idx];
      if (e.sig_cnt) {
        const uint4 *nd = (const uint4 *)(nodes + 8ull * e.sig_first);
        const uint4 r0 = nd[0], r1 = nd[1];
        const uint32_t m[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
        sha256_mix64(h, m);
      } else if (e.mix_off != FDGPU_POH_NO_MIX) {
        uint32_t m[8];
        sha256_load_words<8>(m, arena + e.mix_off, 0u);
        sha256_mix64(h, m);
      }
      uint32_t want[8], diff = 0;
      sha256_load_words<8>(want, arena + e.hash_off, 0u);
#pragma unroll
      for (int j = 0; j < 8; j++) diff |= want[j] ^ h[j];
      poh_store(codes, hashes, idx, diff ? FDGPU_CODE_POH_MISMATCH : 0, h);
      have = false;
    }
  }
}

int poh_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        v < 1)
      v = 256;
    cus = v;
  }
  return cus;
}

}  // namespace

extern "C" {

uint32_t fdgpu_poh_chunk(void) { return FDGPU_POH_CHUNK; }

hipError_t fdgpu_launch_poh_tree(const uint8_t *d_arena, const fdgpu_poh_entry_t *d_entries, uint32_t n,
                                 const uint32_t *d_sig_offs, uint32_t sig_total, uint32_t *d_nodes, hipStream_t stream) {
  if (!n || !sig_total) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_poh_leaf_kernel, dim3((sig_total + 63) / 64), dim3(64), 0, stream, d_arena, d_sig_offs,
                     sig_total, d_nodes);
  hipLaunchKernelGGL(fdgpu_poh_root_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_entries, n, sig_total, d_nodes);
  return hipGetLastError();
}

hipError_t fdgpu_launch_poh_chains(const uint8_t *d_arena, const fdgpu_poh_entry_t *d_entries, uint32_t n,
                                   const uint32_t *d_order, uint32_t n_q, const uint32_t *d_nodes, uint32_t cap,
                                   uint32_t grid_waves, uint32_t *d_head, int8_t *d_codes, uint8_t *d_hashes,
                                   hipStream_t stream) {
  if (!n) return hipSuccess;
  if (cap > FDGPU_POH_HASH_CNT_MAX) cap = FDGPU_POH_HASH_CNT_MAX;
  /* a wave per 64 entries, up to the four per SIMD the kernel's registers allow; the queue feeds the rest */
  const uint32_t most = (uint32_t)poh_cus() * 16u;
  uint32_t waves = grid_waves ? grid_waves : (n + 63u) / 64u;
  if (waves > most) waves = most;
  hipError_t rc = hipMemsetAsync(d_head, 0, sizeof(uint32_t), stream);
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(fdgpu_poh_chain_kernel, dim3((waves * 64u + POH_BLOCK - 1) / POH_BLOCK), dim3(POH_BLOCK), 0, stream,
                     d_arena, d_entries, n, d_order, n_q, d_nodes, cap, waves, d_head, d_codes, d_hashes);
  return hipGetLastError();
}

}  // extern "C"
