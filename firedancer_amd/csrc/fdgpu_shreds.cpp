/* fdgpu_shreds.cpp -- raw Merkle shreds through the engine (include/fd_shred_gpu.h): the ring batch
   (fdgpu_submit_shreds / fdgpu_poll_shreds) and the shred diagnostics.  A batch is its arena uploaded as any frag
   batch's, then on the slot's stream ingest (checks, SHA-256 leaf and proof walk, roots into the arena's roots region,
   one signature descriptor per shred that passed) -> verify -> finish (codes and roots side by side) and one
   read-back. */
#include "fdgpu_engine.h"
#include "fdgpu_shred.h"

using namespace fdgpu;

namespace {

/* The roots region of a batch lies in the arena's own allocation, behind the payload and its slack, so that a
   signature descriptor's 32-bit offsets reach it and the verify reads the roots as it reads any message; `cap` is
   what the allocation holds besides its trailing FDGPU_ARENA_SLACK (which then lies behind the last root).  Checks
   every argument of a shred batch; 0, or FDGPU_ERR_INVAL with the error text set. */
int shred_args(const fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_shred_t const *sh, uint64_t n,
               uint64_t cap, uint64_t *roots_off) {
  if (!e || (!arena && arena_sz) || (!sh && n)) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  if (n > e->cfg.max_txn || n > e->cfg.max_sig || n > 0x7FFFFFFull) { set_err("batch exceeds engine limits"); return FDGPU_ERR_INVAL; }
  for (uint64_t i = 0; i < n; i++)
    if ((uint64_t)sh[i].off + sh[i].sz > arena_sz || (uint64_t)sh[i].pub_off + 32 > arena_sz || sh[i].sz > FDGPU_SHRED_SZ_MAX) {
      set_err("shred %llu: out of the arena, or larger than %u bytes", (unsigned long long)i, FDGPU_SHRED_SZ_MAX);
      return FDGPU_ERR_INVAL;
    }
  *roots_off = (arena_sz + FDGPU_ARENA_SLACK + 15) & ~15ull;
  if (*roots_off + 32 * n > cap) {
    set_err("arena (%llu B), slack and %llu roots exceed the arena allocation (%llu B)", (unsigned long long)arena_sz,
            (unsigned long long)n, (unsigned long long)cap);
    return FDGPU_ERR_INVAL;
  }
  return FDGPU_OK;
}

bool slot_shred_bufs(Slot &s, const fdgpu_cfg_t &c) {
  if (s.d_sh) return true;
  const uint64_t n = c.max_txn + 1;
  HIPCHK(s.h_sh.alloc(n * sizeof(fdgpu_shred_t)), false);
  HIPCHK(s.d_sh_cnt.alloc(64), false);
  HIPCHK(s.d_sh.alloc(n * sizeof(fdgpu_shred_t)), false);
  return true;
}

/* a shred batch resident on the device outside the ring (the diagnostics): synchronous upload */
struct DevShreds {
  DevBuf<uint8_t> arena, res;
  DevBuf<fdgpu_shred_t> sh;
  DevBuf<fdgpu_sig_desc_t> sigs;
  DevBuf<fdgpu_txn_desc_t> tds;
  DevBuf<uint32_t> cnt;
  DevBuf<int8_t> sig_codes;
  uint64_t roots_off = 0;
  int upload(fdgpu_engine_t *e, uint8_t const *a, uint64_t arena_sz, fdgpu_shred_t const *s, uint64_t n) {
    if (!n) { set_err("empty batch"); return FDGPU_ERR_INVAL; }
    const int rc = shred_args(e, a, arena_sz, s, n, UINT32_MAX - 64ull * 1024, &roots_off);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
    /* the roots region behind the arena and its slack, zeroed with them */
    HIPCHK(dev_arena(arena, a, arena_sz, roots_off + 32 * n - arena_sz, false), FDGPU_ERR_DEVICE);
    if (res.alloc(item_results(n).bytes) || sh.alloc(n * sizeof(fdgpu_shred_t)) ||
        sigs.alloc(n * sizeof(fdgpu_sig_desc_t) + 16) || tds.alloc(n * sizeof(fdgpu_txn_desc_t) + 16) || cnt.alloc(64) ||
        sig_codes.alloc(n + 16)) {
      (void)hipGetLastError();
      set_err("alloc");
      return FDGPU_ERR_DEVICE;
    }
    HIPCHK(hipMemcpy(sh, s, n * sizeof(fdgpu_shred_t), hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
    return FDGPU_OK;
  }
  int ingest(uint64_t n, uint16_t version, hipStream_t st) {
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(uint32_t), st), FDGPU_ERR_DEVICE);
    HIPCHK(fdgpu_launch_shred_ingest(arena, sh, (uint32_t)n, version, (uint32_t)roots_off, sigs, tds, cnt, st),
           FDGPU_ERR_DEVICE);
    return FDGPU_OK;
  }
};

}  // namespace

extern "C" {

int64_t fdgpu_submit_shreds(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_shred_t const *sh,
                            uint64_t n, uint16_t expected_version) {
  if (e && arena_sz > e->cfg.max_arena) { set_err("batch exceeds engine limits"); return FDGPU_ERR_INVAL; }
  uint64_t roots_off = 0;
  const int arc = shred_args(e, arena, arena_sz, sh, n, e ? e->cfg.max_arena : 0, &roots_off);
  if (arc) return arc;
  std::lock_guard<std::mutex> lk(e->ring_mu);
  Slot *s = nullptr;
  if (const int rc = take_slot(e, &s)) return rc;
  if (!n) return slot_publish(e, s, Batch::Shred, 0, 0, 0);
  if (!slot_shred_bufs(*s, e->cfg) || !slot_res_bufs(*s, e->cfg) || !slot_ws(*s, n)) return FDGPU_ERR_DEVICE;
  if (const int rc = slot_upload(e, s, arena, arena_sz)) return rc;
  const ItemResults res = item_results(n);
  memcpy(s->h_sh, sh, n * sizeof(fdgpu_shred_t));
  HIPCHK(hipMemcpyAsync(s->d_sh, s->h_sh, n * sizeof(fdgpu_shred_t), hipMemcpyHostToDevice, s->stream), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemsetAsync(s->d_sh_cnt, 0, sizeof(uint32_t), s->stream), FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_shred_ingest(s->d_arena, s->d_sh, (uint32_t)n, expected_version, (uint32_t)roots_off, s->d_sigs,
                                   s->d_txns, s->d_sh_cnt, s->stream),
         FDGPU_ERR_DEVICE);
  /* n bounds the signature count (one per shred that passed); the count itself stays on the device */
  HIPCHK(fdgpu_launch_verify_sigs(s->d_arena, s->d_sigs, (uint32_t)n, nullptr, e->d_btab, s->d_ws, s->d_sig_codes,
                                  ring_kflags(e, s, n), s->stream, s->d_sh_cnt, e->resident_blocks, e->kc_seed),
         FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_shred_finish(s->d_txns, (uint32_t)n, s->d_sig_codes, s->d_arena + roots_off, (int8_t *)s->d_res.p,
                                   s->d_res + res.items, s->stream),
         FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpyAsync(s->h_res, s->d_res, res.bytes, hipMemcpyDeviceToHost, s->stream), FDGPU_ERR_DEVICE);
  return slot_publish(e, s, Batch::Shred, n, 0, 0);
}

int fdgpu_poll_shreds(fdgpu_engine_t *e, int64_t ticket, int8_t *codes, uint8_t *roots, int blocking) {
  return poll_slot(e, ticket, codes, blocking, false, nullptr, nullptr, nullptr, roots);
}

int fdgpu_debug_shred_roots(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_shred_t const *sh,
                            uint64_t n, uint16_t expected_version, int8_t *ok, uint8_t *roots) {
  if (!ok || !roots) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  DevShreds b;
  int rc = b.upload(e, arena, arena_sz, sh, n);
  if (!rc) rc = b.ingest(n, expected_version, e->compute);
  if (rc) return rc;
  HIPCHK(fdgpu_launch_shred_finish(b.tds, (uint32_t)n, nullptr, b.arena + b.roots_off, (int8_t *)b.res.p,
                                   b.res + item_results(n).items, e->compute),
         FDGPU_ERR_DEVICE);
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(ok, b.res, n, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(roots, b.res + item_results(n).items, 32 * n, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

int fdgpu_debug_shred_time(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_shred_t const *sh,
                           uint64_t n, uint16_t expected_version, int iters, double *ingest_ms, double *verify_ms) {
  if (iters < 1 || !ingest_ms || !verify_ms) { set_err("bad argument"); return FDGPU_ERR_INVAL; }
  DevShreds b;
  int rc = b.upload(e, arena, arena_sz, sh, n);
  if (rc) return rc;
  if (n > e->ws_sig) {
    HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
    rc = ensure_ws(e, n);
    if (rc) return rc;
  }
  hipStream_t st = e->compute;
  /* the warm-up also leaves the descriptors and the count the timed verifies read */
  auto ingest = [&] { return !b.ingest(n, expected_version, st); };
  auto verify = [&] {
    return fdgpu_launch_verify_sigs(b.arena, b.sigs, (uint32_t)n, nullptr, e->d_btab, e->d_ws, b.sig_codes, kflags(e), st,
                                    b.cnt, e->resident_blocks, e->kc_seed) == hipSuccess;
  };
  return time_two_stages(st, iters, "shred", [&] { return ingest() && verify(); }, ingest, verify, ingest_ms, verify_ms);
}

}  // extern "C"
