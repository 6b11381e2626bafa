/* fdgpu_diag.cpp -- the fdgpu_debug_* diagnostics that run the kernels' building blocks (field, decode, SHA-512,
   SHA-256, scalar) on caller data, for the parity tests, and the two-stage timer of the fdgpu_debug_*_time ones.
   Synchronous, on the engine's compute stream. */
#include "fdgpu_engine.h"
#include "fdgpu_shred.h"

using namespace fdgpu;

/* n elements of the buffer's type, and a cache line to spare */
#define DALLOC(buf, n) do { if ((buf).alloc((size_t)(n) * sizeof(*(buf).p) + 64) != hipSuccess) { \
  set_err("alloc"); return FDGPU_ERR_DEVICE; } } while (0)

/* n messages of the arena (with their signature and key, sig_pub) through one of the hash test kernels, out_bytes each
   back */
using MsgLaunch = hipError_t (*)(const uint8_t *, const fdgpu_sig_desc_t *, uint32_t, uint32_t *, hipStream_t);
static int debug_msgs(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_txn_t const *txns, uint64_t n,
                      uint8_t *out, MsgLaunch launch, uint64_t out_bytes, bool sig_pub) {
  if (!e || !n) return FDGPU_ERR_INVAL;
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  std::vector<fdgpu_sig_desc_t> d(n);
  for (uint64_t i = 0; i < n; i++) {
    if ((uint64_t)txns[i].msg_off + txns[i].msg_sz > arena_sz ||
        (sig_pub && ((uint64_t)txns[i].sig_off + 64 > arena_sz || (uint64_t)txns[i].pub_off + 32 > arena_sz))) {
      set_err("descriptor out of bounds"); return FDGPU_ERR_INVAL;
    }
    d[i].msg_off = txns[i].msg_off; d[i].msg_sz = txns[i].msg_sz;
    d[i].sig_off = txns[i].sig_off; d[i].pub_off = txns[i].pub_off;
  }
  DevBuf<uint8_t> da;
  DevBuf<fdgpu_sig_desc_t> dd;
  DevBuf<uint8_t> dout;
  HIPCHK(dev_arena(da, arena, arena_sz), FDGPU_ERR_DEVICE);
  DALLOC(dd, n);
  DALLOC(dout, n * out_bytes);
  HIPCHK(hipMemcpy(dd, d.data(), n * sizeof(fdgpu_sig_desc_t), hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
  HIPCHK(launch(da, dd, (uint32_t)n, (uint32_t *)dout.p, e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(out, dout, n * out_bytes, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

/* n elements of in_words u32 each through one of the test kernels, out_words u32 each back */
template <class Launch>
static int debug_map(fdgpu_engine_t *e, uint8_t const *in, uint64_t n, uint64_t in_words, uint64_t out_words,
                     uint8_t *out, Launch launch) {
  if (!e || !n) return FDGPU_ERR_INVAL;
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  DevBuf<uint32_t> din, dout;
  DALLOC(din, n * in_words);
  DALLOC(dout, n * out_words);
  HIPCHK(hipMemcpy(din, in, n * in_words * 4, hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
  HIPCHK(launch(din.p, dout.p, (uint32_t)n, e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(out, dout, n * out_words * 4, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

/* The device time of two stages of a pipeline on st, for fdgpu_debug_<what>_time: one warm-up (it runs both stages,
   and leaves what the second reads of the first), then iters runs of the first between two events and iters of the
   second between the next two; the means in ms.  Every callable answers whether its launches were queued. */
int fdgpu::time_two_stages(hipStream_t st, int iters, const char *what, const std::function<bool()> &warm,
                           const std::function<bool()> &first, const std::function<bool()> &second, double *first_ms,
                           double *second_ms) {
  Events ev;
  if (!ev.create(3)) { (void)hipGetLastError(); set_err("event"); return FDGPU_ERR_DEVICE; }
  bool ok = warm() && hipEventRecord(ev[0], st) == hipSuccess;
  for (int i = 0; i < iters && ok; i++) ok = first();
  ok = ok && hipEventRecord(ev[1], st) == hipSuccess;
  for (int i = 0; i < iters && ok; i++) ok = second();
  ok = ok && hipEventRecord(ev[2], st) == hipSuccess && hipEventSynchronize(ev[2]) == hipSuccess;
  float a = 0.f, b = 0.f;
  ok = ok && hipEventElapsedTime(&a, ev[0], ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev[1], ev[2]) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); set_err("%s timing failed", what); return FDGPU_ERR_DEVICE; }
  *first_ms = a / iters;
  *second_ms = b / iters;
  return FDGPU_OK;
}

extern "C" {

int fdgpu_debug_fe_ops(fdgpu_engine_t *e, uint8_t const *ab, uint64_t n, uint8_t *out) {
  return debug_map(e, ab, n, 16, 64, out, fdgpu_launch_test_fe);
}

int fdgpu_debug_decode(fdgpu_engine_t *e, uint8_t const *enc, uint64_t n, int ref_mapping, uint8_t *out) {
  const uint32_t flags = ref_mapping ? FDGPU_FLAG_REF_MAP : 0u;
  return debug_map(e, enc, n, 8, 18, out, [flags](const uint32_t *i, uint32_t *o, uint32_t k, hipStream_t st) {
    return fdgpu_launch_test_decode(i, o, k, flags, st);
  });
}

int fdgpu_debug_sha512(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_txn_t const *msgs,
                       uint64_t n, uint8_t *out) {
  return debug_msgs(e, arena, arena_sz, msgs, n, out, fdgpu_launch_test_sha512, 64, false);
}

int fdgpu_debug_hram(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_txn_t const *txns,
                     uint64_t n, uint8_t *out) {
  return debug_msgs(e, arena, arena_sz, txns, n, out, fdgpu_launch_test_hram, 32, true);
}

int fdgpu_debug_sha256(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_txn_t const *msgs, uint64_t n,
                       uint8_t *out) {
  if (!e || !n || !msgs || !out || (!arena && arena_sz) || arena_sz > 0xFFFFFF00ull) { set_err("bad argument"); return FDGPU_ERR_INVAL; }
  return debug_msgs(e, arena, arena_sz, msgs, n, out, fdgpu_launch_test_sha256, 32, false);
}

int fdgpu_debug_sc_reduce(fdgpu_engine_t *e, uint8_t const *in, uint64_t n, uint8_t *out) {
  return debug_map(e, in, n, 16, 8, out, fdgpu_launch_test_sc_reduce);
}

int fdgpu_debug_hs_split(fdgpu_engine_t *e, uint8_t const *k, uint64_t n, uint8_t *out) {
  return debug_map(e, k, n, 8, 16, out, fdgpu_launch_test_hs_split);
}

int fdgpu_debug_fe_raw(fdgpu_engine_t *e, uint8_t const *fg, uint64_t n, uint8_t *out) {
  return debug_map(e, fg, n, 20, 80, out, fdgpu_launch_test_fe_raw);
}

int fdgpu_debug_ge_ops(fdgpu_engine_t *e, uint8_t const *in, uint64_t n, uint8_t *out) {
  return debug_map(e, in, n, fdgpu_test_ge_in_words(), 32u * fdgpu_test_ge_results(), out, fdgpu_launch_test_ge);
}

int fdgpu_debug_sc_recode(fdgpu_engine_t *e, uint8_t const *s, uint64_t n, uint8_t *out) {
  return debug_map(e, s, n, 8, 16, out, fdgpu_launch_test_sc_recode);
}

int fdgpu_debug_tabpack(fdgpu_engine_t *e, uint8_t const *in, uint64_t n, uint8_t *out) {
  return debug_map(e, in, n, FDGPU_ATAB_WORDS, FDGPU_TABPACK_OUT_WORDS, out, fdgpu_launch_test_tabpack);
}

int fdgpu_debug_verify_prehashed(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz,
                                 fdgpu_sig_desc_t const *descs, uint64_t n, uint32_t flags, int8_t *codes_out,
                                 uint32_t *n_full_out) {
  if (!e || !e->d_btab || !arena || !descs || !codes_out || !n_full_out || !n || n > (1u << 20) ||
      arena_sz > 0xFFFFFF00ull || (flags & ~(uint32_t)(FDGPU_FLAG_REF_MAP | FDGPU_FLAG_KFULL | FDGPU_FLAG_KPAIR))) {
    set_err("fdgpu_debug_verify_prehashed: bad argument"); return FDGPU_ERR_INVAL;
  }
  for (uint64_t i = 0; i < n; i++) {
    if ((descs[i].msg_off & 7u) || (uint64_t)descs[i].msg_off + 64 > arena_sz ||
        (uint64_t)descs[i].sig_off + 64 > arena_sz || (uint64_t)descs[i].pub_off + 32 > arena_sz) {
      set_err("fdgpu_debug_verify_prehashed: descriptor out of bounds"); return FDGPU_ERR_INVAL;
    }
  }
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  DevBuf<uint8_t> da;
  DevBuf<fdgpu_sig_desc_t> dd;
  DevBuf<int8_t> dc;
  DevBuf<uint32_t> dws;
  HIPCHK(dev_arena(da, arena, arena_sz), FDGPU_ERR_DEVICE);
  DALLOC(dd, n);
  DALLOC(dc, n);
  if (dws.alloc(fdgpu_ws_bytes(n)) != hipSuccess) { set_err("alloc"); return FDGPU_ERR_DEVICE; }
  HIPCHK(hipMemcpy(dd, descs, n * sizeof(fdgpu_sig_desc_t), hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemsetAsync(dc, 0x7f, n, e->compute), FDGPU_ERR_DEVICE);   /* a code no kernel writes */
  HIPCHK(fdgpu_launch_verify_prehashed(da, dd, (uint32_t)n, e->d_btab, dws, dc, flags, e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(codes_out, dc, n, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(n_full_out, fdgpu_ws_layout(dws, n).cnt, sizeof(uint32_t), hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

int fdgpu_debug_btab(fdgpu_engine_t *e, uint64_t first_entry, uint64_t n_entries, uint32_t *out) {
  const uint64_t total = (uint64_t)FDGPU_BCOMB_NDIG * FDGPU_BCOMB_ENTRIES;
  if (!e || !e->d_btab || !out || first_entry > total || n_entries > total - first_entry) {
    set_err("fdgpu_debug_btab: entries out of the table"); return FDGPU_ERR_INVAL;
  }
  if (!n_entries) return FDGPU_OK;
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(out, e->d_btab + first_entry * FDGPU_BCOMB_STRIDE, n_entries * FDGPU_BCOMB_STRIDE * sizeof(uint32_t),
                   hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

uint32_t fdgpu_bcomb_dim(int which) {
  switch (which) {
    case 0: return FDGPU_BCOMB_BITS;
    case 1: return FDGPU_BCOMB_NDIG;
    case 2: return FDGPU_BCOMB_ENTRIES;
    case 3: return FDGPU_BCOMB_STRIDE;
    case 4: return FDGPU_BCOMB_CHUNK;
    default: return 0u;
  }
}

int fdgpu_debug_sig_codes(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_txn_t const *txns,
                          uint64_t txn_cnt, int8_t *sig_codes) {
  if (!e) return FDGPU_ERR_INVAL;
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  uint64_t total = 0;
  for (uint64_t t = 0; t < txn_cnt; t++) total += (txns[t].sig_cnt >= 1 && txns[t].sig_cnt <= 16) ? txns[t].sig_cnt : 0;
  std::vector<fdgpu_sig_desc_t> sd(total + 1);
  std::vector<fdgpu_txn_desc_t> td(txn_cnt + 1);
  std::vector<uint32_t> pm(total + 1);
  uint32_t *perm = bucket(e) ? pm.data() : nullptr;
  const int64_t ns = expand(arena_sz, txns, txn_cnt, total, sd.data(), td.data(), perm);
  if (ns < 0) return FDGPU_ERR_INVAL;
  if (!ns) return FDGPU_OK;
  DevBuf<uint8_t> da;
  DevBuf<fdgpu_sig_desc_t> dd;
  DevBuf<uint32_t> dp;
  DevBuf<int8_t> dc;
  HIPCHK(dev_arena(da, arena, arena_sz), FDGPU_ERR_DEVICE);
  DALLOC(dd, ns);
  DALLOC(dp, ns);
  DALLOC(dc, ns);
  HIPCHK(hipMemcpy(dd, sd.data(), ns * sizeof(fdgpu_sig_desc_t), hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
  if (perm) HIPCHK(hipMemcpy(dp, perm, ns * sizeof(uint32_t), hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
  const uint32_t flags = kflags(e);
  if ((uint64_t)ns > e->ws_sig) { int rc = ensure_ws(e, (uint64_t)ns); if (rc) return rc; }
  HIPCHK(fdgpu_launch_verify_sigs(da, dd, (uint32_t)ns, perm ? dp.p : nullptr, e->d_btab, e->d_ws, dc, flags,
                                  e->compute, nullptr, e->resident_blocks, e->kc_seed),
         FDGPU_ERR_DEVICE);
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(sig_codes, dc, ns, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

}  // extern "C"
