/* fdgpu_secp256k1.hip -- a block's secp256k1 precompile instructions on the
   device (include/fd_secp256k1_gpu.h), unit for unit what fdgpu_precompile.hip
   is for the Ed25519 ones:

     ingest   one transaction per lane, one wave per block: fdt_parse_core
              (fdt_parse.h) into the lane's 852-byte record, a first
              fdt_secp256k1_walk_core (fdt_secp256k1.h, the host library's own
              source) that counts the records that resolve, the wave's slot
              claim -- one inclusive scan of the counts, one atomic add on the
              batch's device-side record count --, and a second walk that
              writes the record descriptors and their positions;
     recover  one record per lane over those descriptors and that count:
              fdt_secp256k1_record_core -- Keccak-256 of the message, the
              public-key recovery, Keccak-256 of the key, the address compare
              -- and one code per record;
     finish   per transaction fdt_secp256k1_verdict_core over its records'
              codes: the code and the 16-byte info side by side for one
              read-back.

   The recover is the work: some 6,300 field products of 64 v_mad_u64_u32
   each per record (256 doublings, up to 256 additions, three 256-step
   exponentiations), against a few thousand instructions for a Keccak block.
   A lane's message loop runs to its own block count, at most
   FDT_SECP256K1_MSG_BLOCKS, so a wave runs to its longest message.  Lanes
   diverge where the scalars' bits differ (an addition or none) and in the
   addition's rare special cases; every branch rejoins within the step. */
#include <hip/hip_runtime.h>

#include "fdgpu_secp256k1.h"
#include "fdt_secp256k1.h"

#ifndef FDG_DEV
#define FDG_DEV __device__ __forceinline__
#endif

namespace {

/* inclusive scan over the wave (as fdgpu_precompile.hip's) */
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

/* the second walk's emitter: record k of the transaction into slot rec0 + k;
   never past the cnt slots the lane claimed */
struct write_emit {
  fdgpu_sig_desc_t *descs;
  uint32_t *pos;
  uint32_t base, slot, end;
  FDG_DEV void operator()(uint32_t j, uint32_t i, uint32_t sig_at, uint32_t addr_at, uint32_t msg_at, uint32_t msg_sz) {
    if (slot < end) {
      *(uint4 *)(descs + slot) = make_uint4(base + msg_at, msg_sz, base + sig_at, base + addr_at);
      pos[slot] = (j << 16) | i;
    }
    slot++;
  }
};

/* fdgpu_precompile_walk_t as one 16-B store / load */
FDG_DEV uint4 walk_pack(uint32_t rec0, uint32_t rec_cnt, uint32_t instr, uint32_t rec, uint32_t k1_cnt, int code) {
  return make_uint4(rec0, (rec_cnt & 0xFFFFu) | (instr << 16), (rec & 0xFFFFu) | (k1_cnt << 16), (uint32_t)(code & 0xFF));
}

__global__ void __launch_bounds__(64) fdgpu_secp256k1_ingest_kernel(const uint8_t *__restrict__ arena,
                                                                    const fdgpu_precompile_t *__restrict__ txns,
                                                                    uint32_t n, uint32_t flags,
                                                                    uint8_t *__restrict__ txn_out,
                                                                    fdgpu_sig_desc_t *__restrict__ descs,
                                                                    uint32_t *__restrict__ pos,
                                                                    uint4 *__restrict__ walks,
                                                                    uint32_t *__restrict__ n_rec) {
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
      fdt_secp256k1_walk_core(payload, pc.sz, t, flags, ce, &w);
    }
  }
  uint32_t cnt = parsed ? w.rec_cnt : 0u;
  const bool capped = cnt > pc.sig_cap;
  if (capped) cnt = 0;
  /* the wave's transactions take consecutive runs of descriptor slots */
  const uint32_t incl = wave_incl_scan(cnt);
  const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
  uint32_t base = 0;
  if ((threadIdx.x & 63u) == 0 && total) base = atomicAdd(n_rec, total);
  base = (uint32_t)__shfl((int)base, 0, 64);
  if (!active) return;
  const uint32_t rec0 = base + incl - cnt;
  if (cnt) {
    write_emit we{descs, pos, pc.off, rec0, rec0 + cnt};
    fdt_precompile_walk_t w2;
    fdt_secp256k1_walk_core(payload, pc.sz, t, flags, we, &w2);
  }
  if (!parsed || capped)
    walks[i] = walk_pack(0, 0, FDT_PRECOMPILE_NONE, FDT_PRECOMPILE_NONE, 0,
                         capped ? FDGPU_CODE_PRECOMPILE_CAP : FDGPU_CODE_PARSE_FAIL);
  else
    walks[i] = walk_pack(rec0, cnt, w.instr_idx, w.rec_idx, w.ed_instr_cnt, w.code);
}

__global__ void __launch_bounds__(64) fdgpu_secp256k1_recover_kernel(const uint8_t *__restrict__ arena,
                                                                     const fdgpu_sig_desc_t *__restrict__ descs,
                                                                     uint32_t cap, const uint32_t *__restrict__ n_rec,
                                                                     int8_t *__restrict__ codes) {
  const uint32_t cnt = *n_rec, n = cnt < cap ? cnt : cap;
  const uint32_t k = blockIdx.x * 64u + threadIdx.x;
  if (k >= n) return;
  const uint4 d = *(const uint4 *)(descs + k);               /* {msg_off, msg_sz, sig_off, addr_off} */
  fdt_precompile_reader r;
  r.p = arena;
  codes[k] = (int8_t)fdt_secp256k1_record_core(r, d.x, d.y, d.z, d.w);
}

__global__ void __launch_bounds__(256) fdgpu_secp256k1_finish_kernel(const uint4 *__restrict__ walks, uint32_t n,
                                                                     const int8_t *__restrict__ rec_codes,
                                                                     const uint32_t *__restrict__ pos,
                                                                     int8_t *__restrict__ codes,
                                                                     uint4 *__restrict__ infos) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint4 w = walks[i];
    const uint32_t rec0 = w.x, rec_cnt = w.y & 0xFFFFu;
    int code = (int)(int8_t)(w.w & 0xFFu);
    fdgpu_precompile_info_t info;
    if (code == FDGPU_CODE_PARSE_FAIL || code == FDGPU_CODE_PRECOMPILE_CAP) fdt_precompile_info_none(&info);
    else
      code = fdt_secp256k1_verdict_core(
          code, w.y >> 16, w.z & 0xFFFFu, w.z >> 16, rec_cnt,
          [&](uint32_t k) { return rec_codes ? (int)rec_codes[rec0 + k] : 0; }, [&](uint32_t k) { return pos[rec0 + k]; },
          &info);
    codes[i] = (int8_t)code;
    infos[i] = make_uint4((uint32_t)info.instr_idx | ((uint32_t)info.rec_idx << 16),
                          (uint32_t)info.ed_instr_cnt | ((uint32_t)info.sig_cnt << 16), (uint32_t)(uint8_t)info.ed_code, 0u);
  }
}

/* ---- test kernels ---- */

__global__ void __launch_bounds__(64) fdgpu_test_keccak256_kernel(const uint8_t *__restrict__ arena,
                                                                  const uint32_t *__restrict__ off_sz, uint32_t n,
                                                                  uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t off = off_sz[2u * i], sz = off_sz[2u * i + 1u];
  fdt_precompile_reader r;
  r.p = arena;
  uint64_t st[25];
  fdt_keccak256_init(st);
  const uint32_t nb0 = fdt_keccak256_block_cnt(sz);
  const uint32_t nb = nb0 < FDT_SECP256K1_MSG_BLOCKS ? nb0 : FDT_SECP256K1_MSG_BLOCKS;
#pragma unroll 1
  for (uint32_t b = 0; b < nb; b++) fdt_keccak256_absorb_block(st, r, off, sz, b);
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) {
    out[8u * i + 2u * k] = (uint32_t)st[k];
    out[8u * i + 2u * k + 1u] = (uint32_t)(st[k] >> 32);
  }
}

__global__ void __launch_bounds__(64) fdgpu_test_secp256k1_recover_kernel(const uint8_t *__restrict__ in, uint32_t n,
                                                                          int8_t *__restrict__ codes,
                                                                          uint32_t *__restrict__ keys) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  fdt_precompile_reader r;
  r.p = in;
  const uint64_t at = 97ull * i;
  fdt_u256 h, sr, ss, x, y;
  fdt_u256_load_be(h, r, at);
  fdt_u256_load_be(sr, r, at + 32u);
  fdt_u256_load_be(ss, r, at + 64u);
  const uint32_t recid = r.at(at + 96u);
  codes[i] = (int8_t)fdt_secp256k1_recover_core(h, sr, ss, recid, x, y);
#pragma unroll
  for (int j = 0; j < 8; j++) {                              /* x | y, big endian */
    keys[16u * i + j] = fdt_bswap32(x.v[7 - j]);
    keys[16u * i + 8 + j] = fdt_bswap32(y.v[7 - j]);
  }
}

FDG_DEV void load_u256(fdt_u256 &a, const uint32_t *p) {
#pragma unroll
  for (int j = 0; j < 8; j++) a.v[j] = p[j];
}

/* the affine point (x, y) under the Jacobian scaling z: (x z^2 : y z^3 : z) */
FDG_DEV void load_point(fdt_k1_point &pt, const uint32_t *p) {
  fdt_u256 x, y, z2, one;
  load_u256(x, p);
  load_u256(y, p + 8);
  load_u256(pt.z, p + 16);
  fdt_u256_set(one, 1u);
  fdt_fe_mul(pt.z, pt.z, one);                               /* reduced, as every coordinate is kept */
  fdt_fe_sqr(z2, pt.z);
  fdt_fe_mul(pt.x, x, z2);
  fdt_fe_mul(z2, z2, pt.z);
  fdt_fe_mul(pt.y, y, z2);
}

__global__ void __launch_bounds__(64) fdgpu_test_secp256k1_ops_kernel(const uint32_t *__restrict__ in,
                                                                      uint32_t *__restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t *p = in + (uint64_t)FDGPU_SECP256K1_OPS_IN * i;
  const uint32_t op = p[0];
  fdt_u256 a, b, x, y;
  load_u256(a, p + 1);
  load_u256(b, p + 9);
  fdt_u256_set(x, 0u);
  fdt_u256_set(y, 0u);
  uint32_t flag = 0;
  if (op == 0u) fdt_fe_mul(x, a, b);
  else if (op == 1u) fdt_fe_sqr(x, a);
  else if (op == 2u) fdt_fe_inv(x, a);
  else if (op == 3u) flag = fdt_fe_sqrt(x, a) ? 1u : 0u;
  else if (op == 4u) fdt_sc_mul(x, a, b);
  else if (op == 5u) fdt_sc_inv(x, a);
  else if (op == 6u) fdt_sc_reduce(x, a);
  else if (op == 7u || op == 8u) {
    fdt_k1_point P, Q, R;
    load_point(P, p + 1);
    if (op == 7u) {
      load_point(Q, p + 25);
      fdt_k1_add(R, P, Q);
    } else {
      fdt_k1_dbl(R, P);
    }
    if (fdt_k1_is_infinity(R)) flag = 1u;
    else fdt_k1_affine(x, y, R);
  }
  uint32_t *o = out + (uint64_t)FDGPU_SECP256K1_OPS_OUT * i;
  o[0] = flag;
#pragma unroll
  for (int j = 0; j < 8; j++) { o[1 + j] = x.v[j]; o[9 + j] = y.v[j]; }
}

}  // namespace

extern "C" {

hipError_t fdgpu_launch_secp256k1_ingest(const uint8_t *d_arena, const fdgpu_precompile_t *d_txns, uint32_t n,
                                         uint32_t flags, uint8_t *d_txn_out, fdgpu_sig_desc_t *d_descs, uint32_t *d_pos,
                                         fdgpu_precompile_walk_t *d_walk, uint32_t *d_n_rec, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_secp256k1_ingest_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_arena, d_txns, n, flags,
                     d_txn_out, d_descs, d_pos, (uint4 *)d_walk, d_n_rec);
  return hipGetLastError();
}

hipError_t fdgpu_launch_secp256k1_recover(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_descs, uint32_t cap,
                                          const uint32_t *d_n_rec, int8_t *d_codes, hipStream_t stream) {
  if (!cap) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_secp256k1_recover_kernel, dim3((cap + 63) / 64), dim3(64), 0, stream, d_arena, d_descs, cap,
                     d_n_rec, d_codes);
  return hipGetLastError();
}

hipError_t fdgpu_launch_secp256k1_finish(const fdgpu_precompile_walk_t *d_walk, uint32_t n, const int8_t *d_rec_codes,
                                         const uint32_t *d_pos, int8_t *d_codes, uint8_t *d_info, hipStream_t stream) {
  if (!n) return hipSuccess;
  const uint32_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(fdgpu_secp256k1_finish_kernel, dim3(blocks < FDGPU_AUX_BLOCKS ? blocks : FDGPU_AUX_BLOCKS),
                     dim3(256), 0, stream, (const uint4 *)d_walk, n, d_rec_codes, d_pos, d_codes, (uint4 *)d_info);
  return hipGetLastError();
}

hipError_t fdgpu_launch_test_keccak256(const uint8_t *d_arena, const uint32_t *d_off_sz, uint32_t n, uint32_t *d_out,
                                       hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_test_keccak256_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_arena, d_off_sz, n, d_out);
  return hipGetLastError();
}

hipError_t fdgpu_launch_test_secp256k1_recover(const uint8_t *d_in, uint32_t n, int8_t *d_codes, uint32_t *d_keys,
                                               hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_test_secp256k1_recover_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_in, n, d_codes,
                     d_keys);
  return hipGetLastError();
}

hipError_t fdgpu_launch_test_secp256k1_ops(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_test_secp256k1_ops_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_in, d_out, n);
  return hipGetLastError();
}

}  // extern "C"
