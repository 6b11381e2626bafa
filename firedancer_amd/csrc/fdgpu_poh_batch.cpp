/* fdgpu_poh_batch.cpp -- a block's proof of history through the engine (include/fd_poh_gpu.h): the ring batch
   (fdgpu_submit_poh / fdgpu_poll_poh) and the PoH diagnostics.  A batch is its arena uploaded as a shred batch's,
   then on the slot's stream the tree (one leaf per signature, one root per entry) -> the chains (one per lane, fed
   from a queue the host orders longest first) and one read-back of [codes, padded to 64][32-B hashes]. */
#include <algorithm>

#include "fdgpu_engine.h"
#include "fdt_poh.h"

using namespace fdgpu;

namespace {

/* Checks every argument of a PoH batch against the entry rules (fdt_poh.h) and the limits given; 0, or
   FDGPU_ERR_INVAL with the error text set. */
int poh_args(const fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_poh_entry_t const *en, uint64_t n,
             uint32_t const *sig_offs, uint64_t sig_total, uint64_t cap, uint64_t max_arena) {
  if (!e || (!arena && arena_sz) || (!en && n) || (!sig_offs && sig_total)) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  if (n > e->cfg.max_txn || sig_total > e->cfg.max_sig || arena_sz > max_arena || n > 0x7FFFFFFull) {
    set_err("batch exceeds engine limits");
    return FDGPU_ERR_INVAL;
  }
  uint64_t bad = 0;
  const int what = fdt_poh_args(arena_sz, en, n, sig_offs, sig_total, cap, &bad);
  if (what) { set_err("poh batch, item %llu: %s", (unsigned long long)bad, fdt_poh_arg_str(what)); return FDGPU_ERR_INVAL; }
  return FDGPU_OK;
}

/* The queue: the entries within the cap, the longest chain first (ties in entry order).  Returns its length. */
uint32_t poh_order(fdgpu_poh_entry_t const *en, uint64_t n, uint64_t cap, uint32_t *order) {
  uint32_t q = 0;
  for (uint64_t i = 0; i < n; i++)
    if (en[i].hash_cnt <= cap) order[q++] = (uint32_t)i;
  std::stable_sort(order, order + q, [en](uint32_t a, uint32_t b) { return en[a].hash_cnt > en[b].hash_cnt; });
  return q;
}

bool slot_poh_bufs(Slot &s, const fdgpu_cfg_t &c) {
  if (s.d_pe) return true;
  const uint64_t n = c.max_txn + 1, ns = c.max_sig + 1;
  HIPCHK(s.h_pe.alloc(n * sizeof(fdgpu_poh_entry_t)), false);
  HIPCHK(s.h_pord.alloc(n * sizeof(uint32_t)), false);
  HIPCHK(s.h_psig.alloc(ns * sizeof(uint32_t)), false);
  HIPCHK(s.d_pord.alloc(n * sizeof(uint32_t)), false);
  HIPCHK(s.d_psig.alloc(ns * sizeof(uint32_t)), false);
  HIPCHK(s.d_pnodes.alloc(ns * 32), false);
  HIPCHK(s.d_phead.alloc(64), false);
  HIPCHK(s.d_pe.alloc(n * sizeof(fdgpu_poh_entry_t)), false);
  return true;
}

/* a PoH batch resident on the device outside the ring (the diagnostics): synchronous upload */
struct DevPoh {
  DevBuf<uint8_t> arena, res;
  DevBuf<fdgpu_poh_entry_t> en;
  DevBuf<uint32_t> sig_offs, order, nodes, head;
  uint32_t n_q = 0;
  int upload(fdgpu_engine_t *e, uint8_t const *a, uint64_t arena_sz, fdgpu_poh_entry_t const *entries, uint64_t n,
             uint32_t const *so, uint64_t sig_total, uint64_t cap) {
    if (!n) { set_err("empty batch"); return FDGPU_ERR_INVAL; }
    const int rc = poh_args(e, a, arena_sz, entries, n, so, sig_total, cap, UINT32_MAX - 64ull * 1024);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device), FDGPU_ERR_DEVICE);
    HIPCHK(dev_arena(arena, a, arena_sz, 0, false), FDGPU_ERR_DEVICE);
    if (res.alloc(item_results(n).bytes) || en.alloc(n * sizeof(fdgpu_poh_entry_t)) ||
        sig_offs.alloc((sig_total + 1) * sizeof(uint32_t)) || order.alloc(n * sizeof(uint32_t)) ||
        nodes.alloc((sig_total + 1) * 32) || head.alloc(64)) {
      (void)hipGetLastError();
      set_err("alloc");
      return FDGPU_ERR_DEVICE;
    }
    std::vector<uint32_t> ord(n);
    n_q = poh_order(entries, n, cap, ord.data());
    HIPCHK(hipMemcpy(en, entries, n * sizeof(fdgpu_poh_entry_t), hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
    if (sig_total) HIPCHK(hipMemcpy(sig_offs, so, sig_total * sizeof(uint32_t), hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
    if (n_q) HIPCHK(hipMemcpy(order, ord.data(), n_q * sizeof(uint32_t), hipMemcpyHostToDevice), FDGPU_ERR_DEVICE);
    return FDGPU_OK;
  }
  bool tree(uint64_t n, uint64_t sig_total, hipStream_t st) {
    return fdgpu_launch_poh_tree(arena, en, (uint32_t)n, sig_offs, (uint32_t)sig_total, nodes, st) == hipSuccess;
  }
  bool chains(uint64_t n, uint64_t cap, uint32_t grid_waves, hipStream_t st) {
    return fdgpu_launch_poh_chains(arena, en, (uint32_t)n, order, n_q, nodes, (uint32_t)cap, grid_waves, head,
                                   (int8_t *)res.p, res + item_results(n).items, st) == hipSuccess;
  }
};

}  // namespace

extern "C" {

int64_t fdgpu_submit_poh(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_poh_entry_t const *entries,
                         uint64_t n, uint32_t const *sig_offs, uint64_t sig_total, uint64_t hash_cnt_cap) {
  const int arc = poh_args(e, arena, arena_sz, entries, n, sig_offs, sig_total, hash_cnt_cap, e ? e->cfg.max_arena : 0);
  if (arc) return arc;
  std::lock_guard<std::mutex> lk(e->ring_mu);
  Slot *s = nullptr;
  if (const int rc = take_slot(e, &s)) return rc;
  if (!n) return slot_publish(e, s, Batch::Poh, 0, 0, 0);
  if (!slot_poh_bufs(*s, e->cfg) || !slot_res_bufs(*s, e->cfg)) return FDGPU_ERR_DEVICE;
  if (const int rc = slot_upload(e, s, arena, arena_sz)) return rc;
  const ItemResults res = item_results(n);
  memcpy(s->h_pe, entries, n * sizeof(fdgpu_poh_entry_t));
  if (sig_total) memcpy(s->h_psig, sig_offs, sig_total * sizeof(uint32_t));
  const uint32_t n_q = poh_order(s->h_pe, n, hash_cnt_cap, s->h_pord);
  HIPCHK(hipMemcpyAsync(s->d_pe, s->h_pe, n * sizeof(fdgpu_poh_entry_t), hipMemcpyHostToDevice, s->stream), FDGPU_ERR_DEVICE);
  if (sig_total)
    HIPCHK(hipMemcpyAsync(s->d_psig, s->h_psig, sig_total * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream),
           FDGPU_ERR_DEVICE);
  if (n_q)
    HIPCHK(hipMemcpyAsync(s->d_pord, s->h_pord, n_q * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream), FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_poh_tree(s->d_arena, s->d_pe, (uint32_t)n, s->d_psig, (uint32_t)sig_total, s->d_pnodes, s->stream),
         FDGPU_ERR_DEVICE);
  HIPCHK(fdgpu_launch_poh_chains(s->d_arena, s->d_pe, (uint32_t)n, s->d_pord, n_q, s->d_pnodes, (uint32_t)hash_cnt_cap, 0,
                                 s->d_phead, (int8_t *)s->d_res.p, s->d_res + res.items, s->stream),
         FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpyAsync(s->h_res, s->d_res, res.bytes, hipMemcpyDeviceToHost, s->stream), FDGPU_ERR_DEVICE);
  return slot_publish(e, s, Batch::Poh, n, 0, 0);
}

int fdgpu_poll_poh(fdgpu_engine_t *e, int64_t ticket, int8_t *codes, uint8_t *hashes, int blocking) {
  return poll_slot(e, ticket, codes, blocking, false, nullptr, nullptr, nullptr, hashes);
}

int fdgpu_poh_limits(fdgpu_engine_t *e, uint64_t *entry_max, uint64_t *sig_max, uint64_t *arena_max) {
  if (!e) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  if (entry_max) *entry_max = e->cfg.max_txn;
  if (sig_max) *sig_max = e->cfg.max_sig;
  if (arena_max) *arena_max = e->cfg.max_arena;
  return FDGPU_OK;
}

int fdgpu_debug_poh(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_poh_entry_t const *entries,
                    uint64_t n, uint32_t const *sig_offs, uint64_t sig_total, uint64_t hash_cnt_cap, uint32_t grid_waves,
                    int8_t *codes, uint8_t *hashes) {
  if (!codes || !hashes) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  DevPoh b;
  const int rc = b.upload(e, arena, arena_sz, entries, n, sig_offs, sig_total, hash_cnt_cap);
  if (rc) return rc;
  if (!b.tree(n, sig_total, e->compute) || !b.chains(n, hash_cnt_cap, grid_waves, e->compute)) {
    (void)hipGetLastError();
    set_err("poh launch failed");
    return FDGPU_ERR_DEVICE;
  }
  HIPCHK(hipStreamSynchronize(e->compute), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(codes, b.res, n, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  HIPCHK(hipMemcpy(hashes, b.res + item_results(n).items, 32 * n, hipMemcpyDeviceToHost), FDGPU_ERR_DEVICE);
  return FDGPU_OK;
}

int fdgpu_debug_poh_time(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_poh_entry_t const *entries,
                         uint64_t n, uint32_t const *sig_offs, uint64_t sig_total, uint64_t hash_cnt_cap, int iters,
                         double *tree_ms, double *chain_ms) {
  if (iters < 1 || !tree_ms || !chain_ms) { set_err("bad argument"); return FDGPU_ERR_INVAL; }
  DevPoh b;
  const int rc = b.upload(e, arena, arena_sz, entries, n, sig_offs, sig_total, hash_cnt_cap);
  if (rc) return rc;
  hipStream_t st = e->compute;
  /* the warm-up also leaves the roots the timed chains read: the fold is in place, so every timed tree run starts
     from the leaves again */
  auto tree = [&] { return b.tree(n, sig_total, st); };
  auto chains = [&] { return b.chains(n, hash_cnt_cap, 0, st); };
  return time_two_stages(st, iters, "poh", [&] { return tree() && chains(); }, tree, chains, tree_ms, chain_ms);
}

}  // extern "C"
