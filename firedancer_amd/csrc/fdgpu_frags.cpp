/* fdgpu_frags.cpp -- the ring's two frag paths, where the device parses the raw payloads: fdgpu_submit_frags
   (payloads uploaded as an arena) and fdgpu_submit_frags_io (payloads gathered from registered host regions, out
   frags written in place), and the merged verify of FDGPU_FLAG_MERGE engines. */
#include <immintrin.h>

#include <algorithm>

#include "fdgpu_engine.h"

using namespace fdgpu;

namespace {

/* Env::submit_prof: where fdgpu_submit_frags_io's time goes (validation loop, enqueue of copies and kernels) */
std::atomic<uint64_t> g_sp_loop{0}, g_sp_enq{0}, g_sp_calls{0}, g_sp_frags{0};

/* the rest of a gathered batch after its verify, from what its submit left in the slot's m_ fields: finish (out frags
   and results written over the bus), the completion word, the done event */
int io_tail(fdgpu_engine_t *e, Slot *s) {
  const uint64_t n = s->m_n;
  const IoResults r = io_results(n);
  HIPCHK(fdgpu_launch_frag_finish_io(s->d_txns, (uint32_t)n, s->d_sig_codes, s->pb.txn_sz, s->d_fxio, s->pb.txn_out,
                                     s->m_arena, s->m_seed, s->m_out, (int8_t *)s->d_trh,
                                     (uint64_t *)(s->d_trh + r.tags), (uint16_t *)(s->d_trh + r.sizes), s->d_io_cnt,
                                     s->stream),
         FDGPU_ERR_DEVICE);
  s->io_cnt_dirty = false;
  return slot_signal(e, s);
}

bool merge_free(const fdgpu_engine_t *e, const Merge &m) {
  if (e->flag_poll) return __atomic_load_n(m.h_flag.p, __ATOMIC_ACQUIRE) == m.seq;
  return !m.seq || hipEventQuery(m.ev[(m.seq - 1) % e->merge_tabs]) == hipSuccess;
}

/* FDGPU_FLAG_MERGE (ring_mu held): the verifies of the batches waiting, as one launch on a merge stream that is idle
   -- or, forced (a blocking poll waits on one of them), on the next one anyway -- then each batch's tail on its own
   stream behind it */
int merge_kick_queue(fdgpu_engine_t *e, bool force) {
  if (e->pending.empty()) return FDGPU_OK;
  if (e->fail_merge_at && ++e->merge_calls == e->fail_merge_at) {
    set_err("injected merge failure (FDGPU_DEBUG_FAIL_MERGE)");
    return FDGPU_ERR_DEVICE;
  }
  const uint32_t nms = (uint32_t)e->merges.size();
  int mi = -1;
  for (uint32_t k = 0; k < nms && mi < 0; k++) {
    const uint32_t j = (e->merge_rr + k) % nms;
    if (merge_free(e, e->merges[j])) mi = (int)j;
  }
  if (mi < 0) {
    if (!force) return FDGPU_OK;
    mi = (int)(e->merge_rr % nms);
  }
  e->merge_rr = (uint32_t)mi + 1;
  Merge &m = e->merges[(size_t)mi];
  const uint32_t ti = m.seq % e->merge_tabs;
  const uint32_t nb = (uint32_t)e->pending.size();
  for (Slot *s : e->pending) HIPCHK(hipStreamWaitEvent(m.stream, s->parsed, 0), FDGPU_ERR_DEVICE);
  if (nb == 1) {                               /* alone: the ring path's kernels (FDGPU_FLAG_PAIR_AUTO applies) */
    Slot *s = e->pending[0];
    HIPCHK(fdgpu_launch_verify_sigs(s->m_arena, s->d_sigs, (uint32_t)s->m_bound, nullptr, e->d_btab, s->d_ws,
                                    s->d_sig_codes, ring_kflags(e, s, s->m_bound), m.stream, s->d_io_cnt,
                                    e->resident_blocks, e->kc_seed, 1),
           FDGPU_ERR_DEVICE);
  } else {
    fdgpu_mbatch_t *tab = m.h_tab + (size_t)ti * e->cfg.ring_depth;
    uint32_t grid_max = 0, slow_max = 0;
    for (uint32_t j = 0; j < nb; j++) {
      Slot *s = e->pending[j];
      const uint32_t grid = (uint32_t)((s->m_bound + FDGPU_BLOCK - 1) / FDGPU_BLOCK);
      uint32_t slow = grid < e->resident_blocks ? grid : e->resident_blocks;
      if (slow > FDGPU_FULL_BLOCKS) slow = FDGPU_FULL_BLOCKS;
      const fdgpu_ws_layout_t l = fdgpu_ws_layout(s->d_ws, s->m_bound);
      st_rlx(s->k_sigs, s->m_bound);
      st_rlx(s->k_lanes, s->m_bound);          /* one lane each: the merged launch never takes the pair kernel */
      tab[j] = fdgpu_mbatch_t{s->m_arena, s->d_sigs, s->d_io_cnt, s->d_ws, s->d_sig_codes,
                              l.queue, l.cnt, (uint32_t)s->m_bound, slow};
      grid_max = grid > grid_max ? grid : grid_max;
      slow_max = slow > slow_max ? slow : slow_max;
    }
    HIPCHK(fdgpu_launch_verify_multi(m.d_tab + (size_t)ti * e->cfg.ring_depth, nb, grid_max, slow_max, e->d_btab,
                                     kflags(e) & ~(uint32_t)FDGPU_FLAG_KPAIR, m.stream),
           FDGPU_ERR_DEVICE);
  }
  HIPCHK(hipEventRecord(m.ev[ti], m.stream), FDGPU_ERR_DEVICE);
  ++m.seq;
  if (e->flag_poll) HIPCHK(hipStreamWriteValue32(m.stream, m.d_flag, m.seq, 0), FDGPU_ERR_DEVICE);
  for (Slot *s : e->pending) {
    HIPCHK(hipStreamWaitEvent(s->stream, m.ev[ti], 0), FDGPU_ERR_DEVICE);
    const int rc = io_tail(e, s);
    if (rc) return rc;
    s->vpending = false;
  }
  e->merge_launches++;
  e->merge_batches += nb;
  e->pending.clear();
  return FDGPU_OK;
}

}  // namespace

namespace fdgpu {

/* a HIP error part-way leaves batches with tickets issued and nothing (or only part) queued for them: each is marked
   failed, so its poll returns the error instead of waiting for a completion word that never comes */
int merge_kick(fdgpu_engine_t *e, bool force) {
  const int rc = merge_kick_queue(e, force);
  if (rc) {
    for (Slot *s : e->pending) if (s->vpending) { s->vpending = false; s->failed = true; }
    e->pending.clear();
  }
  return rc;
}

void submit_prof_report() {
  if (!g_sp_calls) return;
  fprintf(stderr, "[fdgpu submit_frags_io] calls %llu frags %llu: loop %.1f us/call, enqueue %.1f us/call\n",
          (unsigned long long)g_sp_calls.load(), (unsigned long long)g_sp_frags.load(),
          g_sp_loop.load() / 1e3 / g_sp_calls.load(), g_sp_enq.load() / 1e3 / g_sp_calls.load());
}

}  // namespace fdgpu

extern "C" {

/* fdgpu_submit with the parse on the device: upload (DMA from a registered region, or staged), then on the slot's
   stream parse -> scan -> expand -> verify -> combine -> parse-failure codes -> trailer pack, and the codes and
   trailers back to pinned memory. */
int64_t fdgpu_submit_frags(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz, fdgpu_frag_ex_t const *fx,
                           uint64_t n, uint64_t trailer_sz) {
  if (!e || (!arena && arena_sz) || (!fx && n)) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  if (arena_sz > e->cfg.max_arena || n > e->cfg.max_txn) { set_err("batch exceeds engine limits"); return FDGPU_ERR_INVAL; }
  if (trailer_sz > (uint64_t)n * FDT_TXN_MAX_SZ_BYTES + 4) { set_err("trailer buffer larger than the frags' maximum"); return FDGPU_ERR_INVAL; }
  uint64_t bound = 0;
  for (uint64_t t = 0; t < n; t++) {
    const fdgpu_frag_ex_t &f = fx[t];
    if ((uint64_t)f.off + f.sz > arena_sz || (f.tr_off & 3u) || (uint64_t)f.tr_off + f.tr_cap > trailer_sz ||
        f.tr_cap > FDT_TXN_MAX_SZ_BYTES) {
      set_err("frag %llu: out of arena or trailer bounds", (unsigned long long)t);
      return FDGPU_ERR_INVAL;
    }
    bound += fdt_frag_sig_bound(f.sz);
  }
  if (bound > e->cfg.max_sig) { set_err("batch may exceed max_sig (%llu)", (unsigned long long)e->cfg.max_sig); return FDGPU_ERR_INVAL; }
  std::lock_guard<std::mutex> lk(e->ring_mu);
  Slot *s = nullptr;
  if (const int rc = take_slot(e, &s)) return rc;
  if (!slot_frag_bufs(*s, e->cfg, trailer_sz) || !slot_ws(*s, bound)) return FDGPU_ERR_DEVICE;
  if (const int rc = slot_upload(e, s, arena, arena_sz)) return rc;
  const uint64_t tr_base = (n + 63) & ~63ull;
  if (n) {
    ParseBufs &pb = s->pb;
    memcpy(s->h_fx, fx, n * sizeof(fdgpu_frag_ex_t));
    HIPCHK(hipMemcpyAsync(s->d_fx, s->h_fx, n * sizeof(fdgpu_frag_ex_t), hipMemcpyHostToDevice, s->stream), FDGPU_ERR_DEVICE);
    HIPCHK(fdgpu_launch_frag_ring(s->d_arena, s->d_fx, (uint32_t)n, pb.txn_out, pb.txn_sz, pb.txd, pb.cnt, pb.sig0,
                                  pb.blocktot, pb.n_sig, s->d_sigs, s->d_txns, s->stream),
           FDGPU_ERR_DEVICE);
    HIPCHK(fdgpu_launch_verify_sigs(s->d_arena, s->d_sigs, (uint32_t)bound, nullptr, e->d_btab, s->d_ws, s->d_sig_codes,
                                    ring_kflags(e, s, bound), s->stream, pb.n_sig, e->resident_blocks, e->kc_seed),
           FDGPU_ERR_DEVICE);
    HIPCHK(fdgpu_launch_frag_finish(s->d_txns, (uint32_t)n, s->d_sig_codes, pb.txn_sz, s->d_fx, pb.txn_out,
                                    (int8_t *)s->d_tr.p, s->d_tr + tr_base, s->stream),
           FDGPU_ERR_DEVICE);
    HIPCHK(hipMemcpyAsync(s->h_tr, s->d_tr, tr_base + trailer_sz, hipMemcpyDeviceToHost, s->stream), FDGPU_ERR_DEVICE);
  }
  return slot_publish(e, s, Batch::Frag, n, trailer_sz, tr_base);
}

uint32_t fdgpu_frag_out_cap(uint32_t sz) {
  return (uint32_t)(((uint64_t)sz + 1u) / 2u * 2u + fdgpu_frag_fp_bound(sz) + 2u);
}

/* Gathered frag batches (the header's fdgpu_submit_frags_io): the device reads each payload from its registered host
   region (the in dcache) into the slot arena -- and, for a frag naming an in link, re-reads the frag's mcache line
   afterwards (the overrun re-check) -- then parse -> expand -> verify -> finish on the slot's stream; the finish
   kernel writes the out frags into the registered out region and the slot's pinned io_results(), both in place, and
   the stream stores the completion word.  No copies are queued. */
int64_t fdgpu_submit_frags_io(fdgpu_engine_t *e, fdgpu_frag_io_t const *fio, uint64_t n, uint8_t *out,
                              uint64_t out_sz, uint64_t hash_seed, fdgpu_link_t const *links, uint64_t link_cnt) {
  const uint64_t sp0 = g_env.submit_prof ? sp_now() : 0;
  if (!e || (!fio && n) || (!out && out_sz) || (!links && link_cnt)) { set_err("null argument"); return FDGPU_ERR_INVAL; }
  if (n > e->cfg.max_txn) { set_err("batch exceeds engine limits"); return FDGPU_ERR_INVAL; }
  if (link_cnt > FDGPU_LINK_MAX) { set_err("more than %lu links", (unsigned long)FDGPU_LINK_MAX); return FDGPU_ERR_INVAL; }
  std::lock_guard<std::mutex> lk(e->ring_mu);
  const fdgpu_engine::Reg *ro = out_sz ? region_of(e, (uintptr_t)out, out_sz) : nullptr;
  if (out_sz && !ro) { set_err("out range not inside a registered region"); return FDGPU_ERR_UNREG; }
  /* each named link's mcache: its device-side address (the lines are read in place over the bus) */
  uint64_t ldev[FDGPU_LINK_MAX], lmask[FDGPU_LINK_MAX];
  for (uint64_t l = 0; l < link_cnt; l++) {
    const uint64_t d = links[l].depth;
    if (!d || (d & (d - 1)) || (links[l].mcache & 7u)) {
      set_err("link %llu: bad depth or a misaligned mcache", (unsigned long long)l);
      return FDGPU_ERR_INVAL;
    }
    const fdgpu_engine::Reg *rm = region_of(e, (uintptr_t)links[l].mcache, d * 32u);
    if (!rm) {
      set_err("link %llu: mcache not inside a registered region", (unsigned long long)l);
      return FDGPU_ERR_UNREG;
    }
    ldev[l] = rm->dbase + (links[l].mcache - rm->base);
    lmask[l] = d - 1;
  }
  Slot *s = nullptr;
  if (const int rc = take_slot(e, &s)) return rc;
  const IoResults res = io_results(n);         /* in the trailer buffer */
  if (!slot_frag_bufs(*s, e->cfg, res.bytes)) return FDGPU_ERR_DEVICE;
  if (!slot_io_bufs(*s, e->cfg)) return FDGPU_ERR_DEVICE;
  static_assert(sizeof(fdgpu_frag_ex_t) == 16, "one 16-B streaming store per record");
  const IoRecords rec = io_records(n);         /* pinned memory the gather reads in place */
  fdgpu_frag_ex_t *h_fx = (fdgpu_frag_ex_t *)s->h_io.p;
  uint64_t *h_src = (uint64_t *)(s->h_io + rec.src);
  uint64_t *h_chk = (uint64_t *)(s->h_io + rec.chk);
  uint64_t *h_rtab = (uint64_t *)(s->h_io + rec.rtab);
  /* bounds: every payload inside a registered region (16-B aligned: the gather reads 16-B units up to round16(sz),
     inside the payload's own 64-B chunks), every out frag inside out, the packed arena within max_arena, the
     signature bound within max_sig, every named link given.

     DMA gather (Env::io_dma): the frags' payloads are grouped into ranges of source bytes -- per registered region, a
     run of this batch's frags with gaps of at most FDGPU_IO_GAP (a round robin's other tiles' frags lie between this
     tile's) -- and each range is copied into the slot's mirror by the DMA engines; the records then name a range and
     an offset in it, and the payloads are parsed and verified where the copy put them.  More than FDGPU_IO_RANGES_MAX
     ranges, or more bytes than the mirror holds: this batch takes the kernel-load path.

     Measured (engine alone, two engines: 86-89 vs 80-81 M txn/s), yet off by default: in the mux tiles the ranges of
     two tiles sharing a link interleave (each copy carries the other tile's payloads too) and the range building sits
     on the tile's thread -- two tiles 42-59 M with DMA vs 71-72 M without (profiles/r05/aux_blocks.md) */
  struct Range { uintptr_t lo, hi; };
  static thread_local Range rg[FDGPU_IO_RANGES_MAX];
  uint32_t nr = 0;
  uint64_t dev_off = 0, bound = 0;
  bool any_chk = false;
  bool dma = g_env.io_dma && s->d_mirror;
  constexpr uintptr_t FDGPU_IO_GAP = 4096;
  auto fill = [&](bool use_dma) -> int {           /* 0, 1: redo without DMA, < 0: error */
    const fdgpu_engine::Reg *rc = nullptr;
    const fdgpu_engine::Reg *open_reg[16];
    uint32_t open_rng[16], n_open = 0;
    nr = 0; dev_off = 0; bound = 0; any_chk = false;
    for (uint64_t t = 0; t < n; t++) {
      const fdgpu_frag_io_t &f = fio[t];
      const uint64_t q = ((uint64_t)f.sz + 15u) & ~15ull;
      if (f.sz > FDT_TXN_MTU_BYTES || (f.src & 15u) || (f.out_off & 1u) || (uint64_t)f.out_off + f.out_cap > out_sz ||
          f.out_cap > 0xFFFFu || f.link > link_cnt) {
        set_err("frag %llu: size, alignment, out bounds or link", (unsigned long long)t);
        return FDGPU_ERR_INVAL;
      }
      if (!rc || f.src < rc->base || f.src + q > rc->end) rc = region_of(e, (uintptr_t)f.src, q);
      if (!rc) { set_err("frag %llu: payload not inside a registered region", (unsigned long long)t); return FDGPU_ERR_UNREG; }
      uint32_t off, sz = f.sz;
      if (use_dma) {
        uint32_t k = 0;
        while (k < n_open && open_reg[k] != rc) k++;
        uint32_t ri = k < n_open ? open_rng[k] : UINT32_MAX;
        if (ri != UINT32_MAX && f.src >= rg[ri].lo && f.src <= rg[ri].hi + FDGPU_IO_GAP) {
          rg[ri].hi = std::max<uintptr_t>(rg[ri].hi, f.src + q);
        } else {
          if (nr == FDGPU_IO_RANGES_MAX || (k == n_open && n_open == 16)) return 1;
          ri = nr++;
          rg[ri] = Range{(uintptr_t)f.src, (uintptr_t)(f.src + q)};
          if (k == n_open) { open_reg[n_open] = rc; n_open++; }
          open_rng[k] = ri;
        }
        off = (uint32_t)(f.src - rg[ri].lo);
        sz |= ri << 16;
      } else {
        /* streaming stores: the records are for the device (read over the bus), not this core -- no line fills for
           them, nothing to snoop */
        _mm_stream_si64((long long *)&h_src[t], (long long)(rc->dbase + (f.src - rc->base)));
        off = (uint32_t)dev_off;
        dev_off += q;
        if (dev_off > e->cfg.max_arena) { set_err("frags exceed the engine's arena"); return FDGPU_ERR_INVAL; }
      }
      _mm_stream_si128((__m128i *)&h_fx[t], _mm_set_epi32((int)f.out_cap, (int)f.out_off, (int)sz, (int)off));
      if (f.link) {                                       /* {line address, seq}; fd_frag_meta_t.seq: offset 0 */
        _mm_stream_si128((__m128i *)&h_chk[2 * t],
                         _mm_set_epi64x((long long)f.seq, (long long)(ldev[f.link - 1] + (f.seq & lmask[f.link - 1]) * 32u)));
        any_chk = true;
      } else {
        _mm_stream_si64((long long *)&h_chk[2 * t], 0);
      }
      bound += fdt_frag_sig_bound(f.sz);
    }
    if (use_dma) {                                     /* each range's place in the mirror */
      uint64_t m = 0;
      for (uint32_t r = 0; r < nr; r++) {
        h_rtab[r] = m;
        m = (m + (rg[r].hi - rg[r].lo) + 63u) & ~63ull;
      }
      if (m > s->mirror_cap) return 1;
    }
    return 0;
  };
  int frc = fill(dma);
  if (frc == 1) { dma = false; frc = fill(false); }
  if (frc < 0) return frc;
  _mm_sfence();                                        /* the streamed records reach memory before the launches */
  if (bound > e->cfg.max_sig) { set_err("batch may exceed max_sig (%llu)", (unsigned long long)e->cfg.max_sig); return FDGPU_ERR_INVAL; }
  const uint64_t sp1 = g_env.submit_prof ? sp_now() : 0;
  if (!slot_ws(*s, bound)) return FDGPU_ERR_DEVICE;
  /* four kernels: ingest (gather, re-check of the in mcache lines, parse and expand; it keeps the records on the
     device and zeroes the verify queue counter), verify and its fallback, finish -- the out frags and the results
     written in place over the bus -- then the completion word */
  uint8_t *out_dev = out_sz ? (uint8_t *)(ro->dbase + ((uintptr_t)out - ro->base)) : nullptr;
  uint8_t *arena = dma ? s->d_mirror.p : s->d_arena.p;
  if (n) {
    const bool zero_cnt = !(kflags(e) & FDGPU_FLAG_KCACHE);
    for (uint32_t r = 0; dma && r < nr; r++)
      HIPCHK(hipMemcpyAsync(s->d_mirror + h_rtab[r], (const void *)rg[r].lo, rg[r].hi - rg[r].lo, hipMemcpyHostToDevice,
                            s->stream),
             FDGPU_ERR_DEVICE);
    if (s->io_cnt_dirty) HIPCHK(hipMemsetAsync(s->d_io_cnt, 0, 64, s->stream), FDGPU_ERR_DEVICE);
    s->io_cnt_dirty = false;
    HIPCHK(fdgpu_launch_frag_ingest_io((const uint64_t *)(s->d_ioh + rec.src),
                                       (const fdgpu_frag_ex_t *)s->d_ioh,
                                       any_chk ? (const uint64_t *)(s->d_ioh + rec.chk) : nullptr,
                                       dma ? (const uint64_t *)(s->d_ioh + rec.rtab) : nullptr, (uint32_t)n,
                                       arena, s->d_fxio, s->pb.txn_out, s->pb.txn_sz, s->d_sigs, s->d_txns,
                                       s->d_io_cnt,
                                       zero_cnt ? fdgpu_ws_layout(s->d_ws, bound).cnt : nullptr, s->stream),
           FDGPU_ERR_DEVICE);
    s->io_cnt_dirty = true;                            /* until this batch's finish is queued */
    s->m_n = (uint32_t)n; s->m_seed = hash_seed; s->m_out = out_dev; s->m_bound = bound; s->m_arena = arena;
    if (!e->merges.empty() && zero_cnt && bound) {
      /* the verify waits to be merged with the other batches ready (merge_kick): the batch is published first and
         signalled by io_tail, behind the merged launch */
      HIPCHK(hipEventRecord(s->parsed, s->stream), FDGPU_ERR_DEVICE);
      s->vpending = true;
      e->pending.push_back(s);
      const int64_t ticket = slot_publish(e, s, Batch::FragIo, n, 0, 0, true);
      /* a failed merge marks this batch failed: its poll reports the error (returning the error here would leave the
         slot's ticket unknown to the caller, and the slot occupied for good) */
      (void)merge_kick(e, false);
      return ticket;
    }
    HIPCHK(fdgpu_launch_verify_sigs(arena, s->d_sigs, (uint32_t)bound, nullptr, e->d_btab, s->d_ws, s->d_sig_codes,
                                    ring_kflags(e, s, bound), s->stream, s->d_io_cnt, e->resident_blocks, e->kc_seed,
                                    zero_cnt),
           FDGPU_ERR_DEVICE);
    const int rc = io_tail(e, s);
    if (rc) return rc;
  }
  const int64_t ticket = slot_publish(e, s, Batch::FragIo, n, 0, 0, /* io_tail has signalled */ n != 0);
  if (ticket >= 0 && g_env.submit_prof) {
    const uint64_t sp2 = sp_now();
    g_sp_loop += sp1 - sp0; g_sp_enq += sp2 - sp1; g_sp_calls++; g_sp_frags += n;
  }
  return ticket;
}

}  // extern "C"
