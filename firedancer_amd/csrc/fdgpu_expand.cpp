/* fdgpu_expand.cpp -- descriptor expansion and the staging thread pool: host code with no HIP call in it
   (tools/expand_check.cpp compiles this unit alone).  Untrusted descriptors are bounds-checked here before anything
   is handed to the GPU (offsets + sizes must lie inside the arena). */
#include <algorithm>
#include <condition_variable>
#include <thread>

#include "fdgpu_engine.h"

using namespace fdgpu;

namespace {

/* SHA-512 blocks of R || A || M (fdgpu_sha512.h sha512_hram_blocks) */
inline uint32_t hram_blocks(uint32_t msg_sz) { return (64u + msg_sz + 16u) / 128u + 1u; }

/* The staging helpers: FDGPU_COPY_THREADS - 1 process-wide threads started on first use and kept (a thread created
   per submit costs tens of microseconds and was a visible share of a batch's latency tail). */
struct CopyPool {
  std::mutex mu;
  std::condition_variable cv, done_cv;
  std::vector<std::function<void()>> jobs;
  uint64_t pending = 0;
  std::vector<std::thread> th;
  CopyPool() {
    for (unsigned i = 1; i < FDGPU_COPY_THREADS; i++)
      th.emplace_back([this]() {
        for (;;) {
          std::function<void()> job;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [this]() { return !jobs.empty(); });
            job = std::move(jobs.back());
            jobs.pop_back();
          }
          job();
          std::lock_guard<std::mutex> lk(mu);
          if (--pending == 0) done_cv.notify_all();
        }
      });
    for (auto &t : th) t.detach();           /* live for the process */
  }
  /* runs fns[1..] on the pool and fns[0] here; returns when all are done */
  void run(std::vector<std::function<void()>> &fns) {
    {
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 1; i < fns.size(); i++) { jobs.push_back(fns[i]); pending++; }
    }
    cv.notify_all();
    fns[0]();
    std::unique_lock<std::mutex> lk(mu);
    done_cv.wait(lk, [this]() { return pending == 0; });
  }
};
CopyPool &copy_pool() {
  static CopyPool *p = new CopyPool;         /* never destroyed: its threads outlive main */
  return *p;
}
std::mutex g_stage_mu;                       /* one staging at a time uses the pool */

/* expand_par's threshold: below it the serial expand() is the faster one */
constexpr uint64_t FDGPU_EXPAND_SPLIT_MIN = 65536;

}  // namespace

namespace fdgpu {

void copy_run(std::vector<std::function<void()>> &fns) {
  std::lock_guard<std::mutex> lk(g_stage_mu);
  copy_pool().run(fns);
}

/* Validate and expand transactions into per-signature work items.  Returns the number of signatures or -1 on invalid
   input.

   perm != NULL: the descriptors are grouped by SHA-512 block count (a stable counting sort; the SHA loop of a wave
   runs to its longest message, so mixed message sizes in one wave cost the longest one's blocks) and perm[i] is the
   signature index (in transaction order, the combine kernel's sig0 + j) of descriptor i.  perm == NULL: transaction
   order, no permutation. */
int64_t expand(uint64_t arena_sz, const fdgpu_txn_t *txns, uint64_t txn_cnt, uint64_t max_sig,
               fdgpu_sig_desc_t *sigs, fdgpu_txn_desc_t *tds, uint32_t *perm) {
  uint64_t ns = 0;
  uint64_t cnt_by_grp[FDGPU_NBLK_GROUPS] = {};
  for (uint64_t t = 0; t < txn_cnt; t++) {
    const fdgpu_txn_t &x = txns[t];
    const uint32_t cnt = x.sig_cnt;
    tds[t].sig0 = (uint32_t)ns;
    tds[t].sig_cnt = cnt;
    if (cnt == 0 || cnt > 16) { tds[t].sig_cnt = 0; continue; }   /* -> ERR_SIG without verifying */
    if ((uint64_t)x.msg_off + x.msg_sz > arena_sz || (uint64_t)x.sig_off + 64ull * cnt > arena_sz ||
        (uint64_t)x.pub_off + 32ull * cnt > arena_sz) {
      set_err("txn %llu: descriptor out of arena bounds", (unsigned long long)t);
      return -1;
    }
    if (ns + cnt > max_sig) { set_err("batch exceeds max_sig (%llu)", (unsigned long long)max_sig); return -1; }
    if (perm) cnt_by_grp[std::min(hram_blocks(x.msg_sz), FDGPU_NBLK_GROUPS) - 1] += cnt;
    ns += cnt;
  }
  uint64_t next[FDGPU_NBLK_GROUPS];
  if (perm) {
    uint64_t o = 0;
    for (uint32_t g = 0; g < FDGPU_NBLK_GROUPS; g++) { next[g] = o; o += cnt_by_grp[g]; }
  }
  for (uint64_t t = 0; t < txn_cnt; t++) {
    const fdgpu_txn_t &x = txns[t];
    const uint32_t cnt = tds[t].sig_cnt;
    if (!cnt) continue;
    const uint32_t s0 = tds[t].sig0;
    uint64_t *slot = perm ? &next[std::min(hram_blocks(x.msg_sz), FDGPU_NBLK_GROUPS) - 1] : nullptr;
    for (uint32_t j = 0; j < cnt; j++) {
      const uint64_t i = slot ? (*slot)++ : (uint64_t)s0 + j;
      sigs[i].msg_off = x.msg_off;
      sigs[i].msg_sz = x.msg_sz;
      sigs[i].sig_off = x.sig_off + 64u * j;
      sigs[i].pub_off = x.pub_off + 32u * j;
      if (perm) perm[i] = s0 + j;
    }
  }
  return (int64_t)ns;
}

/* expand() over FDGPU_COPY_THREADS parts of the transactions at once, for the large batches whose single-threaded
   expansion (~3 ns a txn, 3 ms for 1 M) sat on the submitting thread beside the staging copy: pass 1 counts and
   validates each part (signatures, block-count groups, the first bad txn), pass 2 writes each part's descriptors at
   its prefix offsets, so the output -- sig0s, descriptors, the stable block-count grouping and its permutation -- is
   byte-identical to expand()'s, and so is the error (the first failing txn in order, of either kind). */
int64_t expand_par(uint64_t arena_sz, const fdgpu_txn_t *txns, uint64_t txn_cnt, uint64_t max_sig,
                   fdgpu_sig_desc_t *sigs, fdgpu_txn_desc_t *tds, uint32_t *perm) {
  if (txn_cnt < FDGPU_EXPAND_SPLIT_MIN) return expand(arena_sz, txns, txn_cnt, max_sig, sigs, tds, perm);
  constexpr unsigned T = FDGPU_COPY_THREADS;
  struct Part {
    uint64_t lo = 0, hi = 0, ns = 0, bad = UINT64_MAX;
    uint64_t grp[FDGPU_NBLK_GROUPS] = {};
  } part[T];
  const uint64_t per = (txn_cnt + T - 1) / T;
  for (unsigned k = 0; k < T; k++) {
    part[k].lo = std::min<uint64_t>(txn_cnt, k * per);
    part[k].hi = std::min<uint64_t>(txn_cnt, part[k].lo + per);
  }
  std::vector<std::function<void()>> fns;
  for (unsigned k = 0; k < T; k++)
    fns.push_back([&, k]() {
      Part &q = part[k];
      for (uint64_t t = q.lo; t < q.hi; t++) {
        const fdgpu_txn_t &x = txns[t];
        const uint32_t cnt = x.sig_cnt;
        tds[t].sig0 = (uint32_t)q.ns;                        /* part-relative until pass 2 */
        tds[t].sig_cnt = cnt;
        if (cnt == 0 || cnt > 16) { tds[t].sig_cnt = 0; continue; }
        if ((uint64_t)x.msg_off + x.msg_sz > arena_sz || (uint64_t)x.sig_off + 64ull * cnt > arena_sz ||
            (uint64_t)x.pub_off + 32ull * cnt > arena_sz) { q.bad = t; return; }
        if (perm) q.grp[std::min(hram_blocks(x.msg_sz), FDGPU_NBLK_GROUPS) - 1] += cnt;
        q.ns += cnt;
      }
    });
  copy_run(fns);
  /* the first failure in transaction order: a part's bad descriptor, or the txn at which the running count passes
     max_sig (expand()'s two checks) */
  uint64_t base = 0;
  for (unsigned k = 0; k < T; k++) {
    const Part &q = part[k];
    const uint64_t end = q.bad == UINT64_MAX ? q.hi : q.bad;
    if (base + q.ns > max_sig || q.bad != UINT64_MAX) {
      uint64_t ns = base;
      for (uint64_t t = q.lo; t < end; t++) {
        const uint32_t c = tds[t].sig_cnt;
        if (ns + c > max_sig) { set_err("batch exceeds max_sig (%llu)", (unsigned long long)max_sig); return -1; }
        ns += c;
      }
      if (q.bad != UINT64_MAX) {
        set_err("txn %llu: descriptor out of arena bounds", (unsigned long long)q.bad);
        return -1;
      }
    }
    base += q.ns;
  }
  uint64_t next[T][FDGPU_NBLK_GROUPS], sig_base[T];
  {
    uint64_t o = 0, gbase[FDGPU_NBLK_GROUPS], acc = 0;
    for (uint32_t g = 0; g < FDGPU_NBLK_GROUPS; g++) {
      gbase[g] = o;
      for (unsigned k = 0; k < T; k++) o += part[k].grp[g];
    }
    for (unsigned k = 0; k < T; k++) {
      sig_base[k] = acc;
      acc += part[k].ns;
      for (uint32_t g = 0; g < FDGPU_NBLK_GROUPS; g++) {
        next[k][g] = gbase[g];
        gbase[g] += part[k].grp[g];
      }
    }
  }
  fns.clear();
  for (unsigned k = 0; k < T; k++)
    fns.push_back([&, k]() {
      const Part &q = part[k];
      uint64_t *nx = next[k];
      for (uint64_t t = q.lo; t < q.hi; t++) {
        const fdgpu_txn_t &x = txns[t];
        const uint32_t s0 = tds[t].sig0 + (uint32_t)sig_base[k];
        tds[t].sig0 = s0;
        const uint32_t cnt = tds[t].sig_cnt;
        if (!cnt) continue;
        uint64_t *slot = perm ? &nx[std::min(hram_blocks(x.msg_sz), FDGPU_NBLK_GROUPS) - 1] : nullptr;
        for (uint32_t j = 0; j < cnt; j++) {
          const uint64_t i = slot ? (*slot)++ : (uint64_t)s0 + j;
          sigs[i].msg_off = x.msg_off;
          sigs[i].msg_sz = x.msg_sz;
          sigs[i].sig_off = x.sig_off + 64u * j;
          sigs[i].pub_off = x.pub_off + 32u * j;
          if (perm) perm[i] = s0 + j;
        }
      }
    });
  copy_run(fns);
  return (int64_t)base;
}

}  // namespace fdgpu
