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

   A set batch (include/fd_shred_sets_gpu.h) takes every shred of its FEC
   sets and spends one verify lane per distinct (signature, root, leader
   key): set ingest -> set dedup -> verify -> set finish, described at the
   kernels below.

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

/* ---------------- set batches (include/fd_shred_sets_gpu.h) ----------------
   Every shred of a batch, one verify lane per distinct (signature, root,
   leader key):

     set ingest  one shred per lane as above -- checks, leaf hash, proof walk,
                 root into the roots region -- but what it records is a state,
                 not a descriptor: rejected, held against a known root (eight
                 dword compares in the lane: match or mismatch), or a
                 candidate for a verify lane;
     set dedup   an open-addressing table of shred indices (the idiom of
                 fdgpu_key_dedup_kernel, fdgpu_verify.hip): a candidate claims
                 an empty slot with atomicCAS after a plain load saw it empty,
                 or compares its 128 key bytes with those of the shred a slot
                 holds.  The roots were written by the previous kernel on the
                 stream and the arena is immutable, so nothing waits on another
                 lane.  After SET_PROBES probes a shred represents itself, which
                 bounds the work under any input.  The representatives take
                 consecutive signature descriptors {msg = root, 32 B, sig =
                 shred, pub}: wave offsets in LDS, one atomic add per workgroup
                 on the batch's device-side count;
     verify      fdgpu_launch_verify_sigs over those descriptors and that count;
     set finish  per shred the code of its state, or of its representative's
                 signature; codes, roots, representatives and the lane count in
                 one block for one read-back. */
#define SET_PROBES 32u
#define SET_EMPTY 0xffffffffu

enum : uint32_t { SET_REJECTED = 0, SET_KNOWN_MATCH = 1, SET_KNOWN_MISMATCH = 2, SET_CANDIDATE = 3 };

__global__ void __launch_bounds__(64) fdgpu_shred_set_ingest_kernel(uint8_t *arena,
                                                                    const fdgpu_set_shred_t *__restrict__ shreds,
                                                                    uint32_t n, uint32_t expected_version,
                                                                    uint32_t roots_off, uint8_t *__restrict__ state) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const fdgpu_set_shred_t sh = shreds[i];
  const uint8_t *shred = arena + sh.off;
  fdt_shred_chk_t chk;
  uint32_t st = SET_REJECTED;
  if (fdt_shred_check_core(shred, sh.sz, (uint16_t)expected_version, &chk)) {
    uint32_t h[8];
    shred_root(h, shred, chk);
    uint4 *dst = (uint4 *)(arena + roots_off + 32ull * i);
    dst[0] = make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]), __builtin_bswap32(h[3]));
    dst[1] = make_uint4(__builtin_bswap32(h[4]), __builtin_bswap32(h[5]), __builtin_bswap32(h[6]), __builtin_bswap32(h[7]));
    st = SET_CANDIDATE;
    if (sh.known_off != FDGPU_SHRED_NO_ROOT) {
      uint32_t k[8], diff = 0;
      sha256_load_words<8>(k, arena + sh.known_off, 0u);     /* big-endian words, as h */
#pragma unroll
      for (int j = 0; j < 8; j++) diff |= k[j] ^ h[j];
      st = diff ? SET_KNOWN_MISMATCH : SET_KNOWN_MATCH;
    }
  }
  state[i] = (uint8_t)st;
}

/* a candidate's key: signature and leader key as words of the arena at any alignment, the root from the (16-B aligned)
   roots region */
struct set_key_t { uint32_t sig[16], pub[8]; uint4 r0, r1; };

FDG_DEV void set_key_load(set_key_t &k, const uint8_t *arena, const fdgpu_set_shred_t &sh, uint32_t roots_off, uint32_t i) {
  sha256_load_words<16>(k.sig, arena + sh.off, 0u);
  sha256_load_words<8>(k.pub, arena + sh.pub_off, 0u);
  const uint4 *r = (const uint4 *)(arena + roots_off + 32ull * i);
  k.r0 = r[0]; k.r1 = r[1];
}

FDG_DEV bool set_key_eq(const set_key_t &a, const set_key_t &b) {
  uint32_t diff = (a.r0.x ^ b.r0.x) | (a.r0.y ^ b.r0.y) | (a.r0.z ^ b.r0.z) | (a.r0.w ^ b.r0.w) |
                  (a.r1.x ^ b.r1.x) | (a.r1.y ^ b.r1.y) | (a.r1.z ^ b.r1.z) | (a.r1.w ^ b.r1.w);
#pragma unroll
  for (int j = 0; j < 16; j++) diff |= a.sig[j] ^ b.sig[j];
#pragma unroll
  for (int j = 0; j < 8; j++) diff |= a.pub[j] ^ b.pub[j];
  return !diff;
}

/* the seeded hash of R (the signature's first 32 bytes) and the root */
FDG_DEV uint32_t set_hash(const set_key_t &k, uint64_t seed) {
  const uint32_t w[16] = {k.sig[0], k.sig[1], k.sig[2], k.sig[3], k.sig[4], k.sig[5], k.sig[6], k.sig[7],
                          k.r0.x,   k.r0.y,   k.r0.z,   k.r0.w,   k.r1.x,   k.r1.y,   k.r1.z,   k.r1.w};
  uint64_t h = seed;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    h ^= ((uint64_t)w[2 * j + 1] << 32) | w[2 * j];
    h *= 0x9e3779b97f4a7c15ull;
    h ^= h >> 29;
  }
  h *= 0xbf58476d1ce4e5b9ull;
  return (uint32_t)(h >> 32) ^ (uint32_t)h;
}

__global__ void __launch_bounds__(256) fdgpu_shred_set_dedup_kernel(const uint8_t *__restrict__ arena,
                                                                    const fdgpu_set_shred_t *__restrict__ shreds,
                                                                    uint32_t n, uint32_t roots_off,
                                                                    const uint8_t *__restrict__ state,
                                                                    uint32_t *__restrict__ ht, uint32_t ht_mask,
                                                                    uint64_t seed, uint32_t *__restrict__ rep_of,
                                                                    uint32_t *__restrict__ slot_of,
                                                                    fdgpu_sig_desc_t *__restrict__ sigs,
                                                                    uint32_t *__restrict__ n_sig) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool is_rep = false;
  fdgpu_set_shred_t sh = {0, 0, 0, 0};
  if (i < n) {
    uint32_t rep = 0xffffffffu;
    if (state[i] == SET_CANDIDATE) {
      sh = shreds[i];
      set_key_t a;
      set_key_load(a, arena, sh, roots_off, i);
      uint32_t slot = set_hash(a, seed) & ht_mask;
      rep = i;
      for (uint32_t p = 0; p < SET_PROBES; p++, slot = (slot + 1u) & ht_mask) {
        /* a plain load first: a set's slot is taken by its first shred, and the
           later ones then compare without an atomic on a hot line */
        uint32_t v = ht[slot];                      /* stale only as EMPTY: the CAS then reads it */
        if (v == SET_EMPTY) {
          v = atomicCAS(&ht[slot], SET_EMPTY, i);
          if (v == SET_EMPTY) break;                /* claimed: i represents its key */
        }
        set_key_t b;
        set_key_load(b, arena, shreds[v], roots_off, v);
        if (set_key_eq(a, b)) { rep = v; break; }
      }
      is_rep = rep == i;
    }
    rep_of[i] = rep;
  }
  /* the representatives' descriptor slots: wave offsets in LDS, one global
     atomic per workgroup (every thread of the block reaches the barriers) */
  __shared__ uint32_t s_cnt, s_base;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const uint64_t m = __ballot(is_rep);
  const int lane = (int)(threadIdx.x & 63u);
  uint32_t wbase = 0;
  if (m && lane == __ffsll((long long)m) - 1) wbase = atomicAdd(&s_cnt, (uint32_t)__popcll(m));
  if (m) wbase = (uint32_t)__shfl((int)wbase, __ffsll((long long)m) - 1, 64);
  __syncthreads();
  if (threadIdx.x == 0) s_base = s_cnt ? atomicAdd(n_sig, s_cnt) : 0u;
  __syncthreads();
  if (is_rep) {
    const uint32_t slot = s_base + wbase + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    fdgpu_sig_desc_t sd;
    sd.msg_off = roots_off + 32u * i;
    sd.msg_sz = 32u;
    sd.sig_off = sh.off;
    sd.pub_off = sh.pub_off;
    sigs[slot] = sd;
    slot_of[i] = slot;
  }
}

__global__ void __launch_bounds__(256) fdgpu_shred_set_finish_kernel(const uint8_t *__restrict__ state,
                                                                     const uint32_t *__restrict__ rep_of,
                                                                     const uint32_t *__restrict__ slot_of, uint32_t n,
                                                                     const int8_t *__restrict__ sig_codes,
                                                                     const uint8_t *__restrict__ roots,
                                                                     const uint32_t *__restrict__ n_sig,
                                                                     int8_t *__restrict__ codes,
                                                                     uint8_t *__restrict__ roots_out,
                                                                     uint32_t *__restrict__ lanes_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *lanes_out = *n_sig;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t st = state[i];
    uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
    int code = FDGPU_CODE_SHRED_REJECT;
    if (st != SET_REJECTED) {
      code = st == SET_KNOWN_MATCH ? 0 : st == SET_KNOWN_MISMATCH ? FDGPU_CODE_SHRED_ROOT_MISMATCH
                                                                  : sig_codes[slot_of[rep_of[i]]];
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

hipError_t fdgpu_launch_shred_set_ingest(uint8_t *d_arena, const fdgpu_set_shred_t *d_shreds, uint32_t n,
                                         uint16_t expected_version, uint32_t roots_off, uint8_t *d_state,
                                         hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_shred_set_ingest_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_arena, d_shreds, n,
                     (uint32_t)expected_version, roots_off, d_state);
  return hipGetLastError();
}

hipError_t fdgpu_launch_shred_set_dedup(const uint8_t *d_arena, const fdgpu_set_shred_t *d_shreds, uint32_t n,
                                        uint32_t roots_off, const uint8_t *d_state, uint32_t *d_ht, uint32_t ht_slots,
                                        uint64_t seed, uint32_t *d_rep_of, uint32_t *d_slot_of, fdgpu_sig_desc_t *d_sigs,
                                        uint32_t *d_n_sig, hipStream_t stream) {
  if (!n) return hipSuccess;
  if (ht_slots < 2ull * n || (ht_slots & (ht_slots - 1u))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fdgpu_shred_set_dedup_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_arena, d_shreds, n,
                     roots_off, d_state, d_ht, ht_slots - 1u, seed, d_rep_of, d_slot_of, d_sigs, d_n_sig);
  return hipGetLastError();
}

hipError_t fdgpu_launch_shred_set_finish(const uint8_t *d_state, const uint32_t *d_rep_of, const uint32_t *d_slot_of,
                                         uint32_t n, const int8_t *d_sig_codes, const uint8_t *d_roots,
                                         const uint32_t *d_n_sig, int8_t *d_codes, uint8_t *d_roots_out,
                                         uint32_t *d_lanes_out, hipStream_t stream) {
  if (!n) return hipSuccess;
  const uint32_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(fdgpu_shred_set_finish_kernel, dim3(blocks < FDGPU_AUX_BLOCKS ? blocks : FDGPU_AUX_BLOCKS), dim3(256),
                     0, stream, d_state, d_rep_of, d_slot_of, n, d_sig_codes, d_roots, d_n_sig, d_codes, d_roots_out,
                     d_lanes_out);
  return hipGetLastError();
}

hipError_t fdgpu_launch_test_sha256(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_msgs, uint32_t n,
                                    uint32_t *d_out, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_test_sha256_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_arena, d_msgs, n, d_out);
  return hipGetLastError();
}

}  // extern "C"
