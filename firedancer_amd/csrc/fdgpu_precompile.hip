/* fdgpu_precompile.hip -- a block's Ed25519 precompile instructions on the
   device (include/fd_precompile_gpu.h): the transaction parse, the walk over
   the record tables of its Ed25519 instructions, and the records the verify
   kernels (fdgpu_verify.hip) take from there.

     ingest  one transaction per lane: fdt_parse_core (fdt_parse.h) into the
             lane's 852-byte record in global memory, a first
             fdt_precompile_walk_core (fdt_precompile.h, the host library's
             own source) that counts the records that resolve, the wave's
             slot claim -- one inclusive scan of the counts, one atomic add
             on the batch's device-side signature count --, and a second walk
             that writes the signature descriptors and their positions;
     verify  fdgpu_launch_verify_sigs over those descriptors and that count;
     finish  per transaction fdt_precompile_verdict_core over its signatures'
             codes: the code and the 16-byte info side by side for one
             read-back.

   A lane's walk is byte reads through fdt_reader's 16-B windows and integer
   compares: at most 64 program-id compares and 255 records of 14 bytes.
   Lanes of a wave differ in their instruction and record counts, so they
   diverge; the work is a few thousand instructions a lane against the
   verify's ~10^6 a signature.  One wave per block keeps the slot claim to a
   scan and one atomic. */
#include <hip/hip_runtime.h>

#include "fdgpu_precompile.h"
#include "fdt_precompile.h"

#ifndef FDG_DEV
#define FDG_DEV __device__ __forceinline__
#endif

namespace {

/* inclusive scan over the wave (as fdgpu_ingest.hip's) */
FDG_DEV uint32_t wave_incl_scan(uint32_t v) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, off, 64);
    v += lane >= off ? u : 0u;
  }
  return v;
}

struct count_emit {
  FDG_DEV void operator()(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {}
};

/* the second walk's emitter: record k of the transaction into slot sig0 + k;
   never past the cnt slots the lane claimed */
struct write_emit {
  fdgpu_sig_desc_t *sigs;
  uint32_t *pos;
  uint32_t base, slot, end;
  FDG_DEV void operator()(uint32_t j, uint32_t i, uint32_t sig_at, uint32_t pub_at, uint32_t msg_at, uint32_t msg_sz) {
    if (slot < end) {
      *(uint4 *)(sigs + slot) = make_uint4(base + msg_at, msg_sz, base + sig_at, base + pub_at);
      pos[slot] = (j << 16) | i;
    }
    slot++;
  }
};

/* fdgpu_precompile_walk_t as one 16-B store / load */
FDG_DEV uint4 walk_pack(uint32_t sig0, uint32_t sig_cnt, uint32_t instr, uint32_t rec, uint32_t ed_cnt, int code) {
  return make_uint4(sig0, (sig_cnt & 0xFFFFu) | (instr << 16), (rec & 0xFFFFu) | (ed_cnt << 16), (uint32_t)(code & 0xFF));
}

__global__ void __launch_bounds__(64) fdgpu_precompile_ingest_kernel(const uint8_t *__restrict__ arena,
                                                                     const fdgpu_precompile_t *__restrict__ txns,
                                                                     uint32_t n, uint8_t *__restrict__ txn_out,
                                                                     fdgpu_sig_desc_t *__restrict__ sigs,
                                                                     uint32_t *__restrict__ pos,
                                                                     uint4 *__restrict__ walks,
                                                                     uint32_t *__restrict__ n_sig) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  const bool active = i < n;
  const fdgpu_precompile_t pc = txns[active ? i : n - 1u];
  const uint8_t *payload = arena + pc.off;
  fdt_txn_t *t = (fdt_txn_t *)(txn_out + (uint64_t)FDT_TXN_MAX_SZ * (active ? i : n - 1u));
  fdt_precompile_walk_t w;
  w.code = FDGPU_CODE_PARSE_FAIL; w.rec_cnt = 0; w.instr_idx = w.rec_idx = (uint16_t)FDT_PRECOMPILE_NONE;
  w.ed_instr_cnt = 0; w._pad = 0;
  bool parsed = false;
  if (active) {
    uint64_t fail;
    parsed = fdt_parse_core(payload, pc.sz, t, &fail) != 0;
    if (parsed) {
      count_emit ce;
      fdt_precompile_walk_core(payload, pc.sz, t, ce, &w);
    }
  }
  uint32_t cnt = parsed ? w.rec_cnt : 0u;
  const bool capped = cnt > pc.sig_cap;
  if (capped) cnt = 0;
  /* the wave's transactions take consecutive runs of descriptor slots */
  const uint32_t incl = wave_incl_scan(cnt);
  const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
  uint32_t base = 0;
  if ((threadIdx.x & 63u) == 0 && total) base = atomicAdd(n_sig, total);
  base = (uint32_t)__shfl((int)base, 0, 64);
  if (!active) return;
  const uint32_t sig0 = base + incl - cnt;
  if (cnt) {
    write_emit we{sigs, pos, pc.off, sig0, sig0 + cnt};
    fdt_precompile_walk_t w2;
    fdt_precompile_walk_core(payload, pc.sz, t, we, &w2);
  }
  if (!parsed || capped)
    walks[i] = walk_pack(0, 0, FDT_PRECOMPILE_NONE, FDT_PRECOMPILE_NONE, 0,
                         capped ? FDGPU_CODE_PRECOMPILE_CAP : FDGPU_CODE_PARSE_FAIL);
  else
    walks[i] = walk_pack(sig0, cnt, w.instr_idx, w.rec_idx, w.ed_instr_cnt, w.code);
}

__global__ void __launch_bounds__(256) fdgpu_precompile_finish_kernel(const uint4 *__restrict__ walks, uint32_t n,
                                                                      const int8_t *__restrict__ sig_codes,
                                                                      const uint32_t *__restrict__ pos,
                                                                      int8_t *__restrict__ codes,
                                                                      uint4 *__restrict__ infos) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint4 w = walks[i];
    const uint32_t sig0 = w.x, sig_cnt = w.y & 0xFFFFu;
    int code = (int)(int8_t)(w.w & 0xFFu);
    fdgpu_precompile_info_t info;
    if (code == FDGPU_CODE_PARSE_FAIL || code == FDGPU_CODE_PRECOMPILE_CAP) fdt_precompile_info_none(&info);
    else
      code = fdt_precompile_verdict_core(
          code, w.y >> 16, w.z & 0xFFFFu, w.z >> 16, sig_cnt,
          [&](uint32_t k) { return sig_codes ? (int)sig_codes[sig0 + k] : 0; }, [&](uint32_t k) { return pos[sig0 + k]; },
          &info);
    codes[i] = (int8_t)code;
    infos[i] = make_uint4((uint32_t)info.instr_idx | ((uint32_t)info.rec_idx << 16),
                          (uint32_t)info.ed_instr_cnt | ((uint32_t)info.sig_cnt << 16), (uint32_t)(uint8_t)info.ed_code, 0u);
  }
}

}  // namespace

extern "C" {

hipError_t fdgpu_launch_precompile_ingest(const uint8_t *d_arena, const fdgpu_precompile_t *d_txns, uint32_t n,
                                          uint8_t *d_txn_out, fdgpu_sig_desc_t *d_sigs, uint32_t *d_pos,
                                          fdgpu_precompile_walk_t *d_walk, uint32_t *d_n_sig, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_precompile_ingest_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_arena, d_txns, n,
                     d_txn_out, d_sigs, d_pos, (uint4 *)d_walk, d_n_sig);
  return hipGetLastError();
}

hipError_t fdgpu_launch_precompile_finish(const fdgpu_precompile_walk_t *d_walk, uint32_t n, const int8_t *d_sig_codes,
                                          const uint32_t *d_pos, int8_t *d_codes, uint8_t *d_info,
                                          hipStream_t stream) {
  if (!n) return hipSuccess;
  const uint32_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(fdgpu_precompile_finish_kernel, dim3(blocks < FDGPU_AUX_BLOCKS ? blocks : FDGPU_AUX_BLOCKS),
                     dim3(256), 0, stream, (const uint4 *)d_walk, n, d_sig_codes, d_pos, d_codes, (uint4 *)d_info);
  return hipGetLastError();
}

}  // extern "C"
