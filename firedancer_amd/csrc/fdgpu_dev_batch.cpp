/* fdgpu_dev_batch.cpp -- device-resident batches (fdgpu_dev_batch_*): a batch uploaded once and verified any number
   of times, on the engine's compute stream or on a queue of its own. */
#include "fdgpu_engine.h"

using namespace fdgpu;

struct __attribute__((visibility("hidden"))) fdgpu_dev_batch {
  DevBuf<uint8_t> d_arena;
  DevBuf<fdgpu_sig_desc_t> d_sigs;
  DevBuf<uint32_t> d_perm;                  /* NULL: descriptors in transaction order */
  DevBuf<fdgpu_txn_desc_t> d_txns;
  DevBuf<int8_t> d_sig_codes, d_txn_codes;
  uint64_t n_sig = 0, n_txn = 0;
  /* fdgpu_dev_batch_own_queue: a private stream + workspace, so verifies of different batches run concurrently (the
     next batch's waves fill the CUs the previous one's last, partial round leaves idle) */
  hipStream_t stream = nullptr;
  DevBuf<uint32_t> d_ws;
  /* frag batches (GPU-side ingest): raw payloads in d_arena; the descriptors above are produced on the device by each
     verify, n_sig is the bound the buffers and the grid are sized for until a codes() call reads the count */
  bool frags = false;
  int device = 0;
  hipStream_t compute = nullptr;            /* the engine's stream (the batch's queue until own_queue) */
  DevBuf<fdgpu_frag_t> d_frags;
  ParseBufs pb;
  uint64_t n_sig_bound = 0;
};

namespace {

hipStream_t batch_stream(fdgpu_engine_t *e, fdgpu_dev_batch_t *b) { return b->stream ? b->stream : e->compute; }
uint32_t *batch_ws(fdgpu_engine_t *e, fdgpu_dev_batch_t *b) { return b->d_ws ? b->d_ws.p : e->d_ws.p; }

/* the ingest kernels of a frag batch (parse -> scan -> expand) on st */
int enqueue_ingest(fdgpu_dev_batch_t *b, hipStream_t st) {
  ParseBufs &pb = b->pb;
  HIPCHK(fdgpu_launch_frag_ingest(b->d_arena, b->d_frags, 2u, (uint32_t)b->n_txn, pb.txn_out, pb.txn_sz, pb.txd, pb.cnt,
                                  pb.sig0, pb.blocktot, pb.n_sig, b->d_sigs, b->d_txns, st),
         FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

}  // namespace

extern "C" {

uint64_t fdgpu_dev_batch_sig_cnt(fdgpu_dev_batch_t const *b) {
  if (!b) return 0;
  if (!b->frags) return b->n_sig;
  uint32_t n = 0;                             /* the count the last verify produced on the device */
  if (hipSetDevice(b->device) != hipSuccess) return 0;
  if (hipStreamSynchronize(b->stream ? b->stream : b->compute) != hipSuccess) return 0;
  if (hipMemcpy(&n, b->pb.n_sig, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return n;
}

int fdgpu_dev_batch_device_ptrs(fdgpu_dev_batch_t const *b, void **d_arena, void **d_sig_desc, void **d_perm,
                                void **d_txn_desc, int8_t **d_sig_codes, int8_t **d_txn_codes) {
  if (!b) return FDGPU_ERR_INVAL;
  if (d_arena) *d_arena = b->d_arena;
  if (d_sig_desc) *d_sig_desc = b->d_sigs;
  if (d_perm) *d_perm = b->d_perm;
  if (d_txn_desc) *d_txn_desc = b->d_txns;
  if (d_sig_codes) *d_sig_codes = b->d_sig_codes;
  if (d_txn_codes) *d_txn_codes = b->d_txn_codes;
  return FDGPU_OK;
}

int fdgpu_dev_batch_own_queue(fdgpu_engine_t *e, fdgpu_dev_batch_t *b) {
  if (!e || !b) return FDGPU_ERR_INVAL;
  if (b->stream) return FDGPU_OK;
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  const uint64_t nsig = b->frags ? b->n_sig_bound : b->n_sig;
  if (b->d_ws.alloc(fdgpu_ws_bytes(nsig ? nsig : 1)) != hipSuccess) { set_err("batch workspace alloc"); return FDGPU_ERR_DEVICE; }
  if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) {
    b->d_ws.reset(); b->stream = nullptr; set_err("batch stream"); return FDGPU_ERR_DEVICE;
  }
  e->batch_streams.push_back(b->stream);
  return FDGPU_OK;
}

void fdgpu_dev_batch_free(fdgpu_engine_t *e, fdgpu_dev_batch_t *b) {
  if (!b) return;
  if (e) { (void)hipSetDevice(e->device); (void)hipStreamSynchronize(e->compute); }
  if (b->stream) {
    (void)hipStreamSynchronize(b->stream);
    if (e) {
      auto &v = e->batch_streams;
      for (size_t i = 0; i < v.size(); i++) if (v[i] == b->stream) { v.erase(v.begin() + (long)i); break; }
    }
    (void)hipStreamDestroy(b->stream);
  }
  delete b;                                   /* its buffers go with their owners */
}

fdgpu_dev_batch_t *fdgpu_dev_batch_upload(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz,
                                          fdgpu_txn_t const *txns, uint64_t txn_cnt) {
  if (!e || (!arena && arena_sz) || (!txns && txn_cnt)) { set_err("null argument"); return nullptr; }
  if (arena_sz > 0xFFFFFFF0ull || txn_cnt > 0xFFFFFFF0ull) { set_err("batch exceeds 32-bit offsets"); return nullptr; }
  HIPCHK(hipSetDevice(e->device), nullptr);
  uint64_t total = 0;
  for (uint64_t t = 0; t < txn_cnt; t++) total += (txns[t].sig_cnt >= 1 && txns[t].sig_cnt <= 16) ? txns[t].sig_cnt : 0;
  std::vector<fdgpu_sig_desc_t> sd(total + 1);
  std::vector<fdgpu_txn_desc_t> td(txn_cnt + 1);
  std::vector<uint32_t> pm(bucket(e) ? total + 1 : 0);
  const int64_t ns = expand(arena_sz, txns, txn_cnt, total, sd.data(), td.data(), bucket(e) ? pm.data() : nullptr);
  if (ns < 0) return nullptr;
  fdgpu_dev_batch *b = new fdgpu_dev_batch();
  b->n_sig = (uint64_t)ns; b->n_txn = txn_cnt;
  auto fail = [&](const char *what) -> fdgpu_dev_batch_t * { set_err("%s", what); fdgpu_dev_batch_free(e, b); return nullptr; };
  if (dev_arena(b->d_arena, arena, arena_sz) != hipSuccess) return fail("arena upload");
  if (b->d_sigs.alloc((ns + 1) * sizeof(fdgpu_sig_desc_t)) != hipSuccess) return fail("sig alloc");
  if (b->d_txns.alloc((txn_cnt + 1) * sizeof(fdgpu_txn_desc_t)) != hipSuccess) return fail("txn alloc");
  if (b->d_sig_codes.alloc(ns + 16) != hipSuccess) return fail("code alloc");
  if (b->d_txn_codes.alloc(txn_cnt + 16) != hipSuccess) return fail("code alloc");
  if (ns && hipMemcpy(b->d_sigs, sd.data(), ns * sizeof(fdgpu_sig_desc_t), hipMemcpyHostToDevice) != hipSuccess) return fail("h2d");
  if (ns && !pm.empty()) {
    if (b->d_perm.alloc(ns * sizeof(uint32_t)) != hipSuccess) return fail("perm alloc");
    if (hipMemcpy(b->d_perm, pm.data(), ns * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return fail("h2d");
  }
  if (txn_cnt && hipMemcpy(b->d_txns, td.data(), txn_cnt * sizeof(fdgpu_txn_desc_t), hipMemcpyHostToDevice) != hipSuccess) return fail("h2d");
  if ((uint64_t)ns > e->ws_sig) {
    if (hipStreamSynchronize(e->compute) != hipSuccess) return fail("sync");
    if (ensure_ws(e, (uint64_t)ns) != FDGPU_OK) { fdgpu_dev_batch_free(e, b); return nullptr; }
  }
  return b;
}

fdgpu_dev_batch_t *fdgpu_dev_batch_upload_frags(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz,
                                                fdgpu_frag_t const *frags, uint64_t frag_cnt) {
  if (!e || (!arena && arena_sz) || (!frags && frag_cnt)) { set_err("null argument"); return nullptr; }
  if (arena_sz > 0xFFFFFFF0ull || frag_cnt > 0x0FFFFFFFull) { set_err("batch exceeds 32-bit offsets"); return nullptr; }
  uint64_t bound = 0;
  for (uint64_t t = 0; t < frag_cnt; t++) {
    if ((uint64_t)frags[t].off + frags[t].sz > arena_sz) {
      set_err("frag %llu out of arena bounds", (unsigned long long)t);
      return nullptr;
    }
    bound += fdgpu_frag_sig_bound(frags[t].sz);
  }
  HIPCHK(hipSetDevice(e->device), nullptr);
  fdgpu_dev_batch *b = new fdgpu_dev_batch();
  b->frags = true;
  b->device = e->device;
  b->compute = e->compute;
  b->n_txn = frag_cnt;
  b->n_sig = bound;
  b->n_sig_bound = bound;
  auto fail = [&](const char *what) -> fdgpu_dev_batch_t * { set_err("%s", what); fdgpu_dev_batch_free(e, b); return nullptr; };
  const uint64_t nt = frag_cnt + 1;
  if (dev_arena(b->d_arena, arena, arena_sz) != hipSuccess) return fail("arena upload");
  if (b->d_frags.alloc(nt * sizeof(fdgpu_frag_t)) != hipSuccess) return fail("frag alloc");
  if (const char *what = b->pb.alloc(frag_cnt)) return fail(what);
  if (b->d_sigs.alloc((bound + 1) * sizeof(fdgpu_sig_desc_t)) != hipSuccess) return fail("sig alloc");
  if (b->d_txns.alloc(nt * sizeof(fdgpu_txn_desc_t)) != hipSuccess) return fail("txn alloc");
  if (b->d_sig_codes.alloc(bound + 16) != hipSuccess) return fail("code alloc");
  if (b->d_txn_codes.alloc(frag_cnt + 16) != hipSuccess) return fail("code alloc");
  if (hipMemset(b->pb.n_sig, 0, sizeof(uint32_t)) != hipSuccess) return fail("memset");
  if (frag_cnt && hipMemcpy(b->d_frags, frags, frag_cnt * sizeof(fdgpu_frag_t), hipMemcpyHostToDevice) != hipSuccess)
    return fail("h2d");
  if (bound > e->ws_sig) {
    if (hipStreamSynchronize(e->compute) != hipSuccess) return fail("sync");
    if (ensure_ws(e, bound) != FDGPU_OK) { fdgpu_dev_batch_free(e, b); return nullptr; }
  }
  return b;
}

int fdgpu_dev_batch_verify(fdgpu_engine_t *e, fdgpu_dev_batch_t *b) {
  if (!e || !b) return FDGPU_ERR_INVAL;
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  if (!b->frags)
    return enqueue_verify(e, b->d_arena, b->d_sigs, b->d_perm, b->n_sig, b->d_txns, b->n_txn, b->d_sig_codes,
                          b->d_txn_codes, batch_stream(e, b), b->d_ws);
  const hipStream_t st = batch_stream(e, b);
  int rc = enqueue_ingest(b, st);
  if (rc) return rc;
  HIPCHK(fdgpu_launch_verify_sigs(b->d_arena, b->d_sigs, (uint32_t)b->n_sig_bound, nullptr, e->d_btab, batch_ws(e, b),
                                  b->d_sig_codes, kflags(e), st, b->pb.n_sig, e->resident_blocks, e->kc_seed),
         FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_combine(b->d_txns, (uint32_t)b->n_txn, b->d_sig_codes, b->d_txn_codes, nullptr, st),
         FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_frag_codes(b->pb.txn_sz, (uint32_t)b->n_txn, b->d_txn_codes, st), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

int fdgpu_dev_batch_txns(fdgpu_engine_t *e, fdgpu_dev_batch_t *b, void *txn_out, uint16_t *txn_sz) {
  if (!e || !b || !b->frags) return FDGPU_ERR_INVAL;
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  HIPCHK(hipStreamSynchronize(batch_stream(e, b)), FDGPU_ERR_DEVICE);
  if (txn_out && b->n_txn)
    HIPCHK(hipMemcpy(txn_out, b->pb.txn_out, b->n_txn * FDT_TXN_MAX_SZ_BYTES, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  if (txn_sz && b->n_txn)
    HIPCHK(hipMemcpy(txn_sz, b->pb.txn_sz, b->n_txn * sizeof(uint16_t), hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

int fdgpu_dev_batch_codes(fdgpu_engine_t *e, fdgpu_dev_batch_t *b, int8_t *txn_codes, int8_t *sig_codes) {
  if (!e || !b) return FDGPU_ERR_INVAL;
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  HIPCHK(hipStreamSynchronize(batch_stream(e, b)), FDGPU_ERR_DEVICE);
  if (b->frags) {                             /* the signature count the verify produced on the device */
    uint32_t n = 0;
    HIPCHK(hipMemcpy(&n, b->pb.n_sig, sizeof(n), hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
    b->n_sig = n;
  }
  if (txn_codes && b->n_txn) HIPCHK(hipMemcpy(txn_codes, b->d_txn_codes, b->n_txn, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  if (sig_codes && b->n_sig) HIPCHK(hipMemcpy(sig_codes, b->d_sig_codes, b->n_sig, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

int fdgpu_dev_batch_time2(fdgpu_engine_t *e, fdgpu_dev_batch_t *b, int iters, double *wall_ms, double *ingest_ms,
                          double *verify_kernel_ms, double *combine_kernel_ms) {
  if (!e || !b || iters < 1) return FDGPU_ERR_INVAL;
  HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
  const uint32_t flags = kflags(e);
  const hipStream_t st = batch_stream(e, b);
  const uint64_t nsig = b->frags ? b->n_sig_bound : b->n_sig;
  if (!b->d_ws && nsig > e->ws_sig) {
    HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
    const int wrc = ensure_ws(e, nsig);
    if (wrc) return wrc;
  }
  Events ev;
  if (!ev.create(4 * (size_t)iters + 1)) { (void)hipGetLastError(); set_err("event"); return FDGPU_ERR_DEVICE; }
  int rc = FDGPU_OK;
  for (int i = 0; i < iters && rc == FDGPU_OK; i++) {
    if (hipEventRecord(ev[4 * i], st) != hipSuccess) rc = FDGPU_ERR_DEVICE;
    if (b->frags && rc == FDGPU_OK) rc = enqueue_ingest(b, st);
    if (hipEventRecord(ev[4 * i + 1], st) != hipSuccess) rc = FDGPU_ERR_DEVICE;
    if (fdgpu_launch_verify_sigs(b->d_arena, b->d_sigs, (uint32_t)nsig, b->d_perm, e->d_btab, batch_ws(e, b),
                                 b->d_sig_codes, flags, st, b->frags ? b->pb.n_sig.p : nullptr, e->resident_blocks,
                                 e->kc_seed) != hipSuccess)
      rc = FDGPU_ERR_DEVICE;
    if (hipEventRecord(ev[4 * i + 2], st) != hipSuccess) rc = FDGPU_ERR_DEVICE;
    if (fdgpu_launch_combine(b->d_txns, (uint32_t)b->n_txn, b->d_sig_codes, b->d_txn_codes, nullptr, st) != hipSuccess)
      rc = FDGPU_ERR_DEVICE;
    if (b->frags && fdgpu_launch_frag_codes(b->pb.txn_sz, (uint32_t)b->n_txn, b->d_txn_codes, st) != hipSuccess)
      rc = FDGPU_ERR_DEVICE;
    if (hipEventRecord(ev[4 * i + 3], st) != hipSuccess) rc = FDGPU_ERR_DEVICE;
  }
  if (rc == FDGPU_OK && hipEventSynchronize(ev[4 * (iters - 1) + 3]) != hipSuccess) rc = FDGPU_ERR_DEVICE;
  double si = 0, sv = 0, sc = 0;
  float ms = 0;
  for (int i = 0; rc == FDGPU_OK && i < iters; i++) {
    (void)hipEventElapsedTime(&ms, ev[4 * i], ev[4 * i + 1]); si += ms;
    (void)hipEventElapsedTime(&ms, ev[4 * i + 1], ev[4 * i + 2]); sv += ms;
    (void)hipEventElapsedTime(&ms, ev[4 * i + 2], ev[4 * i + 3]); sc += ms;
  }
  if (rc == FDGPU_OK) {
    (void)hipEventElapsedTime(&ms, ev[0], ev[4 * (iters - 1) + 3]);
    if (wall_ms) *wall_ms = ms;
    if (ingest_ms) *ingest_ms = b->frags ? si / iters : 0.0;
    if (verify_kernel_ms) *verify_kernel_ms = sv / iters;
    if (combine_kernel_ms) *combine_kernel_ms = sc / iters;
  } else {
    set_err("timing launch failed");
  }
  return rc;
}

/* for a frag batch the ingest kernels count in *verify_kernel_ms */
int fdgpu_dev_batch_time(fdgpu_engine_t *e, fdgpu_dev_batch_t *b, int iters, double *wall_ms, double *verify_kernel_ms,
                         double *combine_kernel_ms) {
  double ig = 0, v = 0;
  const int rc = fdgpu_dev_batch_time2(e, b, iters, wall_ms, &ig, &v, combine_kernel_ms);
  if (rc == FDGPU_OK && verify_kernel_ms) *verify_kernel_ms = v + ig;
  return rc;
}

}  // extern "C"
