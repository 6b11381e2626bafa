/* fdgpu_ingest.hip -- GPU-side ingest.
   Raw transaction payloads -> the verify's descriptors, on the device:
     parse   one payload per lane through fdt_parse_core (fdt_parse.h, the
             host parser's own source): the fd_txn_t (which the verify tile
             writes into its output trailer), its footprint (0: not a
             transaction), and the signature layout -- signatures at
             signature_off, the signer keys are the first sig_cnt account
             addresses, the message runs from message_off to the end;
     scan    exclusive prefix sum of the per-txn signature counts (a count
             outside [1,16] contributes none: batch_single_msg rejects the
             txn unverified, fd_ed25519_user.c:238-241) -> each txn's first
             signature and the batch's signature count, left on the device;
     expand  the per-signature descriptors, in transaction order;
   and, after the verify, the kernels that end a frag batch (finish, codes).
   A valid txn with s signatures is at least 96 s + 38 bytes (s signatures,
   s signer keys, blockhash, the counts), which bounds the signature count
   of a batch from its frag sizes alone (fdgpu_frag_sig_bound). */
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include "fdgpu_internal.h"
#include "fdt_hash.h"
#include "fdt_parse.h"

#ifndef FDG_DEV
#define FDG_DEV __device__ __forceinline__
#endif

namespace {

#define FDGPU_SCAN_BLOCK 1024u      /* txns per scan block: 256 threads x 4 */


/* frag t's {off, sz} are the first two words of a record of `stride` words
   (fdgpu_frag_t: 2, fdgpu_frag_ex_t: 4) */
__global__ void __launch_bounds__(64) fdgpu_frag_parse_kernel(
    const uint8_t *__restrict__ arena, const uint32_t *__restrict__ frags, uint32_t stride, uint32_t n,
    uint8_t *__restrict__ txn_out, uint16_t *__restrict__ txn_sz, fdgpu_txn_t *__restrict__ txd,
    uint32_t *__restrict__ cnt) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const fdgpu_frag_t f = *(const fdgpu_frag_t *)(frags + (size_t)t * stride);
  fdt_txn_t *x = (fdt_txn_t *)(txn_out + (size_t)t * FDT_TXN_MAX_SZ);
  uint64_t why = 0;
  uint64_t fp = fdt_parse_core(arena + f.off, f.sz, x, &why);
  const uint32_t sc = fp ? x->signature_cnt : 0u;
  uint32_t c = (sc >= 1u && sc <= 16u) ? sc : 0u;
  if (c > fdt_frag_sig_bound(f.sz)) { c = 0u; fp = 0u; }       /* cannot happen for a parsed txn (see above) */
  fdgpu_txn_t d;
  d.msg_off = fp ? f.off + x->message_off : f.off;
  d.msg_sz = fp ? f.sz - x->message_off : 0u;
  d.sig_off = fp ? f.off + x->signature_off : f.off;
  d.pub_off = fp ? f.off + x->acct_addr_off : f.off;
  d.sig_cnt = fp ? sc : 0u;
  txd[t] = d;
  cnt[t] = c;
  txn_sz[t] = (uint16_t)fp;
}

/* Inclusive scan of v over the 64 lanes of a wave */
FDG_DEV uint32_t wave_incl_scan(uint32_t v) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, off, 64);
    v += lane >= off ? u : 0u;
  }
  return v;
}

/* Block-local exclusive scan of cnt over FDGPU_SCAN_BLOCK txns -> sig0
   (local), the block's total -> blocktot */
__global__ void __launch_bounds__(256) fdgpu_scan_local_kernel(const uint32_t *__restrict__ cnt, uint32_t n,
                                                               uint32_t *__restrict__ sig0,
                                                               uint32_t *__restrict__ blocktot) {
  __shared__ uint32_t s_wave[4];
  const uint32_t base = blockIdx.x * FDGPU_SCAN_BLOCK + threadIdx.x * 4u;
  uint32_t v[4], sum = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) { v[k] = base + k < n ? cnt[base + k] : 0u; sum += v[k]; }
  const uint32_t incl = wave_incl_scan(sum);
  const uint32_t wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 63u) s_wave[wv] = incl;
  __syncthreads();
  uint32_t off = incl - sum;
  for (uint32_t w = 0; w < wv; w++) off += s_wave[w];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (base + k < n) sig0[base + k] = off;
    off += v[k];
  }
  if (threadIdx.x == 255u) blocktot[blockIdx.x] = off;
}

/* One block: exclusive scan of the nb block totals (in place) and the
   grand total -> *n_sig */
__global__ void __launch_bounds__(1024) fdgpu_scan_blocks_kernel(uint32_t *__restrict__ blocktot, uint32_t nb,
                                                                 uint32_t *__restrict__ n_sig) {
  __shared__ uint32_t s_wave[16];
  __shared__ uint32_t s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (uint32_t b0 = 0; b0 < nb; b0 += 1024u) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t v = i < nb ? blocktot[i] : 0u;
    const uint32_t incl = wave_incl_scan(v);
    const uint32_t wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) s_wave[wv] = incl;
    __syncthreads();
    uint32_t off = s_carry + incl - v;
    for (uint32_t w = 0; w < wv; w++) off += s_wave[w];
    __syncthreads();
    if (i < nb) blocktot[i] = off;
    if (threadIdx.x == 1023u) s_carry = off + v;
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_sig = s_carry;
}

/* One thread per txn: its combine item and its signatures' descriptors */
__global__ void __launch_bounds__(256) fdgpu_frag_expand_kernel(
    const fdgpu_txn_t *__restrict__ txd, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ sig0,
    const uint32_t *__restrict__ blockoff, uint32_t n, fdgpu_sig_desc_t *__restrict__ sigs,
    fdgpu_txn_desc_t *__restrict__ tds) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t c = cnt[t], s0 = sig0[t] + blockoff[t / FDGPU_SCAN_BLOCK];
  fdgpu_txn_desc_t td;
  td.sig0 = s0;
  td.sig_cnt = c;
  tds[t] = td;
  if (!c) return;
  const fdgpu_txn_t d = txd[t];
  for (uint32_t j = 0; j < c; j++) {
    fdgpu_sig_desc_t sd;
    sd.msg_off = d.msg_off;
    sd.msg_sz = d.msg_sz;
    sd.sig_off = d.sig_off + 64u * j;
    sd.pub_off = d.pub_off + 32u * j;
    sigs[s0 + j] = sd;
  }
}

/* Ring-slot frag batches of up to FDGPU_SMALL_SCAN_MAX txns: the
   signature-count scan and the descriptor expansion in ONE block (1024
   threads, each a run of consecutive txns), instead of the three-kernel
   multi-block scan: a verify tile's batch costs two launches fewer. */
__global__ void __launch_bounds__(1024) fdgpu_frag_scan_expand_small_kernel(
    const fdgpu_txn_t *__restrict__ txd, const uint32_t *__restrict__ cnt, uint32_t n,
    fdgpu_sig_desc_t *__restrict__ sigs, fdgpu_txn_desc_t *__restrict__ tds, uint32_t *__restrict__ n_sig) {
  __shared__ uint32_t s_wave[16];
  const uint32_t per = (n + 1023u) / 1024u, t0 = threadIdx.x * per, t1 = min(n, t0 + per);
  uint32_t sum = 0;
  for (uint32_t t = t0; t < t1; t++) sum += cnt[t];
  const uint32_t incl = wave_incl_scan(sum);
  const uint32_t wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 63u) s_wave[wv] = incl;
  __syncthreads();
  uint32_t off = incl - sum;
  for (uint32_t w = 0; w < wv; w++) off += s_wave[w];
  if (threadIdx.x == 1023u) *n_sig = off + sum;
  for (uint32_t t = t0; t < t1; t++) {
    const uint32_t c = cnt[t];
    fdgpu_txn_desc_t td;
    td.sig0 = off;
    td.sig_cnt = c;
    tds[t] = td;
    if (c) {
      const fdgpu_txn_t d = txd[t];
      for (uint32_t j = 0; j < c; j++) {
        fdgpu_sig_desc_t sd;
        sd.msg_off = d.msg_off;
        sd.msg_sz = d.msg_sz;
        sd.sig_off = d.sig_off + 64u * j;
        sd.pub_off = d.pub_off + 32u * j;
        sigs[off + j] = sd;
      }
    }
    off += c;
  }
}

/* The end of a ring-slot frag batch in one launch, per txn: the
   batch_single_msg combine of its signatures' codes, FDGPU_CODE_PARSE_FAIL
   for a payload that is not a transaction, and its parsed fd_txn_t copied
   to the place the caller reserved (from the payload's counts,
   fdt_txn_peek) -- a footprint other than the reservation (only a caller
   bug can cause one) gets FDGPU_CODE_TRAILER_CAP and no verdict.  codes and
   trailers are one buffer (trailers after the codes), copied back in one
   transfer.  Lane per txn; tr_off is 4-byte aligned, the txn record starts
   a 852-B (4-aligned) stride. */
__global__ void __launch_bounds__(256) fdgpu_frag_finish_kernel(const fdgpu_txn_desc_t *__restrict__ txns, uint32_t n,
                                                                const int8_t *__restrict__ sig_codes,
                                                                const uint16_t *__restrict__ txn_sz,
                                                                const fdgpu_frag_ex_t *__restrict__ fx,
                                                                const uint8_t *__restrict__ txn_out,
                                                                int8_t *__restrict__ codes, uint8_t *__restrict__ trailers) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t fp = txn_sz[t];
  int code = -1;
  if (!fp) {
    code = FDGPU_CODE_PARSE_FAIL;
  } else {
    const fdgpu_frag_ex_t f = fx[t];
    if (fp != f.tr_cap) {
      code = FDGPU_CODE_TRAILER_CAP;
    } else {
      const fdgpu_txn_desc_t d = txns[t];
      if (d.sig_cnt >= 1 && d.sig_cnt <= 16) {           /* else ERR_SIG (fd_ed25519_user.c:238-241) */
        int first_struct = 0, any_msg = 0;
        for (uint32_t j = 0; j < d.sig_cnt; j++) {
          const int c = sig_codes[d.sig0 + j];
          if (c == -3) any_msg = 1;
          else if (c != 0 && first_struct == 0) first_struct = c;
        }
        code = first_struct ? first_struct : (any_msg ? -3 : 0);
      }
      const uint32_t *src = (const uint32_t *)(txn_out + (size_t)t * FDT_TXN_MAX_SZ);
      uint32_t *dst = (uint32_t *)(trailers + f.tr_off);
      for (uint32_t w = 0; w < (fp + 3u) / 4u; w++) dst[w] = src[w];
    }
  }
  codes[t] = (int8_t)code;
}

/* Gathered frag batches (fdgpu_submit_frags_io).  Both kernels run on at
   most FDGPU_IO_BLOCKS blocks (fdgpu_internal.h: a workgroup beside the
   verify holds a verify block's slot while it waits on the bus) and each wave
   strides over groups of 64 frags, lane i of a group owning frag 64 g + i. */

/* the group's lane that owns flattened unit k: the first lane whose
   inclusive unit count exceeds k (incl is non-decreasing over the lanes) */
FDG_DEV uint32_t unit_owner(uint32_t incl, uint32_t k) {
  uint32_t o = 0;
#pragma unroll
  for (uint32_t b = 32; b; b >>= 1)
    if ((uint32_t)__shfl((int)incl, (int)(o + b - 1u), 64) <= k) o += b;
  return o;
}

/* Ingest: per group, lane i reads frag i's record and payload address from
   the slot's pinned upload buffer (one coalesced read of each over the bus),
   then the wave copies the group's payloads from host memory (the registered
   in dcache, read in place) to their packed, 16-B aligned places in the batch
   arena -- the payloads' 16-B units flattened over the group, four loads in
   flight per lane (the units past sz lie in the payload's own 64-B chunks).
   With chk, a frag whose pair {line, seq} names an in-mcache line is then
   re-checked as the reference's mux re-checks after its copy (fd_mux.c:
   641-655): once the wave's payload loads have returned, the line's seq is
   read again over the bus (a system-scope load: no cache in between); any
   other value than the frag's seq means the producer republished the line,
   so its payload may have been rewritten under the read, and the record is
   kept with FDGPU_FX_LAPPED set (no parse, no verdict).  An agent-scope
   acquire (L1 invalidate) then makes the copied bytes visible to the
   group's own loads, and lane i parses frag i (fd_txn_parse,
   fdgpu_frag_parse_kernel's parse) and the wave takes its run of descriptor
   slots with one atomic add on *n_sig, so the descriptors stay dense in
   [0, n_sig) grouped by wave (every txn records its own first slot).  The
   records are kept on the device (fx_dev) for the finish kernel; the first
   thread clears the verify kernel's queue counter (zero_word). */
__global__ void __launch_bounds__(256) fdgpu_frag_ingest_io_kernel(
    const uint64_t *__restrict__ src, const fdgpu_frag_ex_t *__restrict__ fx, const uint64_t *__restrict__ chk,
    const uint64_t *__restrict__ rtab, uint32_t n, uint8_t *__restrict__ arena, fdgpu_frag_ex_t *__restrict__ fx_dev,
    uint8_t *__restrict__ txn_out, uint16_t *__restrict__ txn_sz, fdgpu_sig_desc_t *__restrict__ sigs,
    fdgpu_txn_desc_t *__restrict__ tds, uint32_t *__restrict__ n_sig, uint32_t *__restrict__ zero_word) {
  const uint32_t lane = threadIdx.x & 63u, wpb = blockDim.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0 && zero_word) *zero_word = 0u;
  for (uint32_t g = blockIdx.x * wpb + (threadIdx.x >> 6); g * 64u < n; g += gridDim.x * wpb) {
    const uint32_t f = g * 64u + lane;
    const bool act = f < n;
    fdgpu_frag_ex_t x = act ? fx[f] : fdgpu_frag_ex_t{0u, 0u, 0u, 0u};
    const uint64_t line = (act && chk) ? chk[2u * f] : 0ull;
    const uint64_t seq = line ? chk[2u * f + 1u] : 0ull;
    if (rtab && act) {                                  /* DMA gather: the payload is in the arena already */
      x.off = (uint32_t)(rtab[x.sz >> 16] + x.off);
      x.sz &= 0xFFFFu;
    }
    const uint64_t s = (act && !rtab) ? src[f] : 0ull;
    const uint32_t nq = rtab ? 0u : (x.sz + 15u) >> 4;
    const uint32_t incl = wave_incl_scan(nq), excl = incl - nq;
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
    /* unit k of the group: its owner lane's source and arena place (all
       lanes take part in the shuffles; a lane past the end reads the last
       unit's arena place instead of the bus, and stores nothing) */
    auto unit = [&](uint32_t k, const uint4 *&sp, uint4 *&dp) {
      const uint32_t kk = k < total ? k : total - 1u;
      const uint32_t o = unit_owner(incl, kk);
      const uint32_t u = kk - (uint32_t)__shfl((int)excl, (int)o, 64);
      sp = (const uint4 *)(uint64_t)__shfl((long long)s, (int)o, 64) + u;
      dp = (uint4 *)(arena + (uint32_t)__shfl((int)x.off, (int)o, 64)) + u;
      if (k >= total) sp = dp;
    };
    for (uint32_t k0 = 0; k0 < total; k0 += 256u) {
      const uint4 *s0, *s1, *s2, *s3;
      uint4 *d0, *d1, *d2, *d3;
      unit(k0 + lane, s0, d0);
      unit(k0 + 64u + lane, s1, d1);
      unit(k0 + 128u + lane, s2, d2);
      unit(k0 + 192u + lane, s3, d3);
      const uint4 v0 = *s0, v1 = *s1, v2 = *s2, v3 = *s3;       /* four loads over the bus in flight */
      if (k0 + lane < total) *d0 = v0;
      if (k0 + 64u + lane < total) *d1 = v1;
      if (k0 + 128u + lane < total) *d2 = v2;
      if (k0 + 192u + lane < total) *d3 = v3;
    }
    /* every payload load of the wave has returned (and every copy store is
       done: vmcnt counts both on gfx9) before a line is re-read */
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (line) {
      const uint64_t cur = __hip_atomic_load((const uint64_t *)line, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (cur != seq) x.tr_cap |= FDGPU_FX_LAPPED;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      /* this CU's L1 holds none of the old arena bytes */
    uint32_t c = 0;
    fdgpu_txn_t dt{};
    if (act) {
      fx_dev[f] = x;
      fdt_txn_t *t = (fdt_txn_t *)(txn_out + (size_t)f * FDT_TXN_MAX_SZ);
      uint64_t why = 0;
      /* a lapped payload may be torn: not parsed */
      uint64_t fp = (x.tr_cap & FDGPU_FX_LAPPED) ? 0u : fdt_parse_core(arena + x.off, x.sz, t, &why);
      const uint32_t sc = fp ? t->signature_cnt : 0u;
      c = (sc >= 1u && sc <= 16u) ? sc : 0u;
      if (c > fdt_frag_sig_bound(x.sz)) { c = 0u; fp = 0u; }      /* cannot happen for a parsed txn */
      if (fp) {
        dt.msg_off = x.off + t->message_off;
        dt.msg_sz = x.sz - t->message_off;
        dt.sig_off = x.off + t->signature_off;
        dt.pub_off = x.off + t->acct_addr_off;
      }
      txn_sz[f] = (uint16_t)fp;
    }
    const uint32_t ci = wave_incl_scan(c);
    const uint32_t ct = (uint32_t)__shfl((int)ci, 63, 64);
    uint32_t base = 0;
    if (lane == 63u && ct) base = atomicAdd(n_sig, ct);
    base = (uint32_t)__shfl((int)base, 63, 64);
    if (!act) continue;
    const uint32_t s0 = base + ci - c;
    fdgpu_txn_desc_t td;
    td.sig0 = s0;
    td.sig_cnt = c;
    tds[f] = td;
    for (uint32_t j = 0; j < c; j++) {
      fdgpu_sig_desc_t sd;
      sd.msg_off = dt.msg_off;
      sd.msg_sz = dt.msg_sz;
      sd.sig_off = dt.sig_off + 64u * j;
      sd.pub_off = dt.pub_off + 32u * j;
      sigs[s0 + j] = sd;
    }
  }
}

/* bytes b, b+1 (b even) of a frag's out frag [payload sz][pad to 2]
   [fd_txn_t fp][u16 sz] as one 16-bit word: the payload (16-B aligned in
   the arena), the fd_txn_t (4-B aligned record, toff even) and the size
   word all split on even offsets, so every half is one aligned 2-B load */
FDG_DEV uint32_t out_frag_half(uint32_t b, const uint8_t *pl, uint32_t sz, uint32_t toff, const uint8_t *tr,
                               uint32_t fp) {
  if (b < toff) {
    const uint32_t v = *(const uint16_t *)(pl + b);
    return b + 1u < sz ? v : v & 0xffu;                 /* the pad byte of an odd payload */
  }
  if (b < toff + fp) return *(const uint16_t *)(tr + (b - toff));
  return b == toff + fp ? sz & 0xffffu : 0u;
}

/* Finish: per group, lane i writes frag i's code (the batch_single_msg
   combine of its signatures; FDGPU_CODE_PARSE_FAIL; FDGPU_CODE_LAPPED;
   FDGPU_CODE_TRAILER_CAP when the out frag would not fit the caller's
   reservation), its dedup tag (fd_hash of the first signature,
   fd_verify.h:66) and its out size (coalesced over the lanes); then the wave
   writes the group's out frags as fd_verify.c:93-136 lays them out in the
   out dcache -- [payload][pad to 2][fd_txn_t][u16 payload_sz] -- one 16-B
   unit per lane and step, the units flattened over the group: a unit inside
   the payload is one 16-B load from the arena, the others are assembled
   byte by byte; a unit that would pass the frag's reservation (or an out
   frag not 16-B aligned) is written in 2-B stores up to the frag's end.  The
   first thread clears the slot's ingest counter for its next gathered batch
   (zero_next; the verify that read it is complete).  (A completion word
   stored by the kernel's last block was tried: the system-scope fence each
   block then needs writes back the L2 under the concurrent verify kernels
   and halved the tile's rate; the stream's own write after the kernel
   stays.) */
__global__ void __launch_bounds__(256) fdgpu_frag_finish_io_kernel(
    const fdgpu_txn_desc_t *__restrict__ txns, uint32_t n, const int8_t *__restrict__ sig_codes,
    const uint16_t *__restrict__ txn_sz, const fdgpu_frag_ex_t *__restrict__ fx, const uint8_t *__restrict__ txn_out,
    const uint8_t *__restrict__ arena, uint64_t seed, uint8_t *__restrict__ out, int8_t *__restrict__ codes,
    uint64_t *__restrict__ tags, uint16_t *__restrict__ out_szs, uint32_t *__restrict__ zero_next) {
  const uint32_t lane = threadIdx.x & 63u, wpb = blockDim.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0 && zero_next) *zero_next = 0u;
  for (uint32_t g = blockIdx.x * wpb + (threadIdx.x >> 6); g * 64u < n; g += gridDim.x * wpb) {
    const uint32_t f = g * 64u + lane;
    const bool act = f < n;
    uint32_t fp = 0, osz = 0, toff = 0;
    fdgpu_frag_ex_t x{0u, 0u, 0u, 0u};            /* off: arena, sz, tr_off: out offset, tr_cap: its room */
    bool fits = false;
    if (act) {
      fp = txn_sz[f];
      x = fx[f];
      const bool lapped = (x.tr_cap & FDGPU_FX_LAPPED) != 0u;   /* fp is 0 then */
      toff = (x.sz + 1u) & ~1u;
      osz = toff + fp + 2u;
      fits = fp && osz <= x.tr_cap;
      const fdt_txn_t *t = (const fdt_txn_t *)(txn_out + (size_t)f * FDT_TXN_MAX_SZ);
      int code = lapped ? FDGPU_CODE_LAPPED : FDGPU_CODE_PARSE_FAIL;
      uint64_t tag = 0;
      if (fp) {
        tag = fdt_hash_core(seed, arena + x.off + t->signature_off, 64);
        if (!fits) {
          code = FDGPU_CODE_TRAILER_CAP;
        } else {
          code = -1;
          const fdgpu_txn_desc_t d = txns[f];
          if (d.sig_cnt >= 1 && d.sig_cnt <= 16) {           /* else ERR_SIG (fd_ed25519_user.c:238-241) */
            int first_struct = 0, any_msg = 0;
            for (uint32_t j = 0; j < d.sig_cnt; j++) {
              const int c = sig_codes[d.sig0 + j];
              if (c == -3) any_msg = 1;
              else if (c != 0 && first_struct == 0) first_struct = c;
            }
            code = first_struct ? first_struct : (any_msg ? -3 : 0);
          }
        }
      }
      codes[f] = (int8_t)code;
      tags[f] = tag;
      out_szs[f] = (uint16_t)(fits ? osz : 0u);
    }
    const uint32_t nu = fits ? (osz + 15u) >> 4 : 0u;
    const uint32_t incl = wave_incl_scan(nu), excl = incl - nu;
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
    for (uint32_t k0 = 0; k0 < total; k0 += 64u) {       /* wave-uniform: every lane takes part in the shuffles */
      const uint32_t k = k0 + lane < total ? k0 + lane : total - 1u;
      const uint32_t o = unit_owner(incl, k);
      const uint32_t u = k - (uint32_t)__shfl((int)excl, (int)o, 64);
      const uint32_t off = (uint32_t)__shfl((int)x.off, (int)o, 64), sz = (uint32_t)__shfl((int)x.sz, (int)o, 64);
      const uint32_t oof = (uint32_t)__shfl((int)x.tr_off, (int)o, 64);
      const uint32_t cap = (uint32_t)__shfl((int)x.tr_cap, (int)o, 64) & 0xFFFFu;
      const uint32_t ofp = (uint32_t)__shfl((int)fp, (int)o, 64), oosz = (uint32_t)__shfl((int)osz, (int)o, 64);
      const uint32_t otoff = (sz + 1u) & ~1u, b0 = 16u * u;
      const uint8_t *pl = arena + off;
      const uint8_t *tr = txn_out + (size_t)(g * 64u + o) * FDT_TXN_MAX_SZ;
      uint8_t *dst = out + oof + b0;
      if (k0 + lane >= total) continue;
      if (b0 + 16u <= cap && !(((uintptr_t)dst) & 15u)) {
        uint4 w;
        if (b0 + 16u <= sz) {
          w = *(const uint4 *)(pl + b0);                      /* arena offsets are 16-B aligned */
        } else {
          uint32_t q[4];
#pragma unroll
          for (int i = 0; i < 4; i++)
            q[i] = out_frag_half(b0 + 4u * i, pl, sz, otoff, tr, ofp) |
                   (out_frag_half(b0 + 4u * i + 2u, pl, sz, otoff, tr, ofp) << 16);
          w = make_uint4(q[0], q[1], q[2], q[3]);
        }
        *(uint4 *)dst = w;
      } else {
        for (uint32_t b = b0; b < b0 + 16u && b < oosz; b += 2u)
          *(uint16_t *)(out + oof + b) = (uint16_t)out_frag_half(b, pl, sz, otoff, tr, ofp);
      }
    }
  }
}

/* After the combine: a payload that did not parse gets FDGPU_CODE_PARSE_FAIL */
__global__ void __launch_bounds__(256) fdgpu_frag_codes_kernel(const uint16_t *__restrict__ txn_sz, uint32_t n,
                                                               int8_t *__restrict__ codes) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n && !txn_sz[t]) codes[t] = (int8_t)FDGPU_CODE_PARSE_FAIL;
}

}  // namespace

extern "C" {

/* one attribute query: the runtime loads a unit's code object at the first
   use of one of its kernels, and engine open wants that before the first
   frag batch */
hipError_t fdgpu_ingest_load(void) {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, (const void *)fdgpu_frag_parse_kernel);
}

uint64_t fdgpu_frag_sig_bound(uint32_t sz) { return fdt_frag_sig_bound(sz); }

hipError_t fdgpu_launch_frag_ingest(const uint8_t *d_arena, const void *d_frags, uint32_t frag_stride, uint32_t n,
                                    uint8_t *d_txn_out, uint16_t *d_txn_sz, fdgpu_txn_t *d_txd, uint32_t *d_cnt,
                                    uint32_t *d_sig0, uint32_t *d_blocktot, uint32_t *d_n_sig,
                                    fdgpu_sig_desc_t *d_sigs, fdgpu_txn_desc_t *d_tds, hipStream_t stream) {
  if (!n) return hipMemsetAsync(d_n_sig, 0, sizeof(uint32_t), stream);
  const uint32_t nb = (n + FDGPU_SCAN_BLOCK - 1) / FDGPU_SCAN_BLOCK;
  hipLaunchKernelGGL(fdgpu_frag_parse_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_arena,
                     (const uint32_t *)d_frags, frag_stride, n, d_txn_out,
                     d_txn_sz, d_txd, d_cnt);
  hipLaunchKernelGGL(fdgpu_scan_local_kernel, dim3(nb), dim3(256), 0, stream, d_cnt, n, d_sig0, d_blocktot);
  hipLaunchKernelGGL(fdgpu_scan_blocks_kernel, dim3(1), dim3(1024), 0, stream, d_blocktot, nb, d_n_sig);
  hipLaunchKernelGGL(fdgpu_frag_expand_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_txd, d_cnt, d_sig0,
                     d_blocktot, n, d_sigs, d_tds);
  return hipGetLastError();
}

hipError_t fdgpu_launch_frag_codes(const uint16_t *d_txn_sz, uint32_t n, int8_t *d_codes, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_frag_codes_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_txn_sz, n, d_codes);
  return hipGetLastError();
}

hipError_t fdgpu_launch_frag_ring(const uint8_t *d_arena, const fdgpu_frag_ex_t *d_fx, uint32_t n, uint8_t *d_txn_out,
                                  uint16_t *d_txn_sz, fdgpu_txn_t *d_txd, uint32_t *d_cnt, uint32_t *d_sig0,
                                  uint32_t *d_blocktot, uint32_t *d_n_sig, fdgpu_sig_desc_t *d_sigs,
                                  fdgpu_txn_desc_t *d_tds, hipStream_t stream) {
  if (!n) return hipMemsetAsync(d_n_sig, 0, sizeof(uint32_t), stream);
  if (n > FDGPU_SMALL_SCAN_MAX)
    return fdgpu_launch_frag_ingest(d_arena, d_fx, 4u, n, d_txn_out, d_txn_sz, d_txd, d_cnt, d_sig0, d_blocktot,
                                    d_n_sig, d_sigs, d_tds, stream);
  hipLaunchKernelGGL(fdgpu_frag_parse_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, d_arena,
                     (const uint32_t *)d_fx, 4u, n, d_txn_out, d_txn_sz, d_txd, d_cnt);
  hipLaunchKernelGGL(fdgpu_frag_scan_expand_small_kernel, dim3(1), dim3(1024), 0, stream, d_txd, d_cnt, n, d_sigs,
                     d_tds, d_n_sig);
  return hipGetLastError();
}

hipError_t fdgpu_launch_frag_finish(const fdgpu_txn_desc_t *d_tds, uint32_t n, const int8_t *d_sig_codes,
                                    const uint16_t *d_txn_sz, const fdgpu_frag_ex_t *d_fx, const uint8_t *d_txn_out,
                                    int8_t *d_codes, uint8_t *d_trailers, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_frag_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_tds, n, d_sig_codes,
                     d_txn_sz, d_fx, d_txn_out, d_codes, d_trailers);
  return hipGetLastError();
}

uint64_t fdgpu_frag_fp_bound(uint32_t sz) { return fdt_frag_fp_bound(sz); }

static uint32_t env_u32(const char *k, uint32_t d) {
  const char *v = getenv(k);
  return v && atoi(v) > 0 ? (uint32_t)atoi(v) : d;
}
static const uint32_t g_aux_in = env_u32("FDGPU_AUX_BLOCKS_IN", FDGPU_IO_BLOCKS);
static const uint32_t g_aux_fin = env_u32("FDGPU_AUX_BLOCKS_FIN", FDGPU_IO_BLOCKS);
static uint32_t aux_blocks(uint32_t n, uint32_t cap = FDGPU_AUX_BLOCKS) {   /* waves of 64 frags, 4 per block */
  const uint32_t b = (n + 255u) / 256u;
  return b < cap ? b : cap;
}

hipError_t fdgpu_launch_frag_ingest_io(const uint64_t *d_src, const fdgpu_frag_ex_t *d_fx, const uint64_t *d_chk,
                                       const uint64_t *d_rtab, uint32_t n, uint8_t *d_arena,
                                       fdgpu_frag_ex_t *d_fx_dev, uint8_t *d_txn_out, uint16_t *d_txn_sz,
                                       fdgpu_sig_desc_t *d_sigs, fdgpu_txn_desc_t *d_tds, uint32_t *d_n_sig,
                                       uint32_t *d_zero_word, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_frag_ingest_io_kernel, dim3(aux_blocks(n, g_aux_in)), dim3(256), 0, stream, d_src, d_fx, d_chk,
                     d_rtab, n, d_arena, d_fx_dev, d_txn_out, d_txn_sz, d_sigs, d_tds, d_n_sig, d_zero_word);
  return hipGetLastError();
}

hipError_t fdgpu_launch_frag_finish_io(const fdgpu_txn_desc_t *d_tds, uint32_t n, const int8_t *d_sig_codes,
                                       const uint16_t *d_txn_sz, const fdgpu_frag_ex_t *d_fx, const uint8_t *d_txn_out,
                                       const uint8_t *d_arena, uint64_t hash_seed, uint8_t *d_out, int8_t *d_codes,
                                       uint64_t *d_tags, uint16_t *d_out_szs, uint32_t *d_zero_next,
                                       hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(fdgpu_frag_finish_io_kernel, dim3(aux_blocks(n, g_aux_fin)), dim3(256), 0, stream, d_tds, n, d_sig_codes,
                     d_txn_sz, d_fx, d_txn_out, d_arena, hash_seed, d_out, d_codes, d_tags, d_out_szs, d_zero_next);
  return hipGetLastError();
}

}  // extern "C"
