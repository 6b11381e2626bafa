/* fdt_poh.h -- the entry rules of the PoH check (include/fd_poh_gpu.h), stated
   once for the engine's host code (fdgpu_poh_batch.cpp: the argument checks and the
   queue order) and the tile library (tile/fdt_callers.cpp: the host path),
   and a host computation of an entry over fdt_sha256.h.  The reference:
   fd_runtime_poh_verify_wide_task (src/flamenco/runtime/fd_runtime.c:
   2274-2330), fd_poh_append / fd_poh_mixin (src/ballet/poh/fd_poh.c),
   fd_wbmtree32 (src/ballet/bmtree/fd_wbmtree.c). */
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/fd_poh_gpu.h"
#include "fdt_sha256.h"

/* what is wrong with a batch's arguments (0: nothing); *bad = the entry */
enum {
  FDT_POH_ARG_OK = 0,
  FDT_POH_ARG_CAP,        /* hash_cnt_cap outside [1, FDGPU_POH_HASH_CNT_MAX] */
  FDT_POH_ARG_HASH_RANGE, /* prev, hash or mix: 32 bytes outside the arena */
  FDT_POH_ARG_SIG_RANGE,  /* signatures outside sig_offs */
  FDT_POH_ARG_MIX_AND_SIG,
  FDT_POH_ARG_SIG_OFF,    /* a signature's 64 bytes outside the arena */
  FDT_POH_ARG_SIG_ORDER,  /* signature ranges not ascending and disjoint in entry order */
};

static inline const char *fdt_poh_arg_str(int what) {
  switch (what) {
    case FDT_POH_ARG_CAP: return "hash_cnt_cap outside [1, FDGPU_POH_HASH_CNT_MAX]";
    case FDT_POH_ARG_HASH_RANGE: return "a 32-byte hash range lies outside the arena";
    case FDT_POH_ARG_SIG_RANGE: return "the entry's signatures lie outside sig_offs";
    case FDT_POH_ARG_MIX_AND_SIG: return "mix_off set together with sig_cnt";
    case FDT_POH_ARG_SIG_OFF: return "a signature's 64 bytes lie outside the arena";
    case FDT_POH_ARG_SIG_ORDER: return "the entries' signature ranges are not ascending and disjoint";
    default: return "ok";
  }
}

static inline int fdt_poh_args(uint64_t arena_sz, const fdgpu_poh_entry_t *en, uint64_t n, const uint32_t *sig_offs,
                               uint64_t sig_total, uint64_t cap, uint64_t *bad) {
  uint64_t sig_next = 0;   /* the end of the last signature range: the device folds each range in place */
  *bad = 0;
  if (cap < 1 || cap > FDGPU_POH_HASH_CNT_MAX) return FDT_POH_ARG_CAP;
  for (uint64_t i = 0; i < n; i++) {
    const fdgpu_poh_entry_t *e = en + i;
    *bad = i;
    if ((uint64_t)e->prev_off + 32 > arena_sz || (uint64_t)e->hash_off + 32 > arena_sz) return FDT_POH_ARG_HASH_RANGE;
    if (e->mix_off != FDGPU_POH_NO_MIX) {
      if (e->sig_cnt) return FDT_POH_ARG_MIX_AND_SIG;
      if ((uint64_t)e->mix_off + 32 > arena_sz) return FDT_POH_ARG_HASH_RANGE;
    }
    if (e->sig_cnt) {
      if ((uint64_t)e->sig_first + e->sig_cnt > sig_total) return FDT_POH_ARG_SIG_RANGE;
      if (e->sig_first < sig_next) return FDT_POH_ARG_SIG_ORDER;
      sig_next = (uint64_t)e->sig_first + e->sig_cnt;
    }
  }
  for (uint64_t j = 0; j < sig_total; j++) {
    *bad = j;
    if ((uint64_t)sig_offs[j] + 64 > arena_sz) return FDT_POH_ARG_SIG_OFF;
  }
  return FDT_POH_ARG_OK;
}

/* which of append, mixin and root applies */
static inline int fdt_poh_mixes(const fdgpu_poh_entry_t *e) { return e->sig_cnt || e->mix_off != FDGPU_POH_NO_MIX; }
/* the hashes of its chain (before the mixin, if any) */
static inline uint64_t fdt_poh_chain_len(const fdgpu_poh_entry_t *e) {
  return fdt_poh_mixes(e) ? (e->hash_cnt ? e->hash_cnt - 1 : 0) : e->hash_cnt;
}

/* ---- the host computation ---- */

static inline void fdt_poh_store(uint8_t out[32], const uint32_t h[8]) {
  for (int i = 0; i < 8; i++) {
    out[4 * i] = (uint8_t)(h[i] >> 24); out[4 * i + 1] = (uint8_t)(h[i] >> 16);
    out[4 * i + 2] = (uint8_t)(h[i] >> 8); out[4 * i + 3] = (uint8_t)h[i];
  }
}

/* fd_poh_append: the block is the hash, the 0x80 and the length 256, built once */
static inline void fdt_poh_append(uint8_t poh[32], uint64_t n) {
  uint8_t blk[64];
  memset(blk, 0, sizeof blk);
  memcpy(blk, poh, 32);
  blk[32] = 0x80; blk[62] = 0x01;
  fdt_sha256_t s;
  while (n--) {
    fdt_sha256_init(&s);
    fdt_sha256_block(s.h, blk);
    fdt_poh_store(blk, s.h);
  }
  memcpy(poh, blk, 32);
}

/* SHA-256 of parts a (an) then b (bn) */
static inline void fdt_poh_sha2(uint8_t out[32], const uint8_t *a, size_t an, const uint8_t *b, size_t bn) {
  fdt_sha256_t s;
  fdt_sha256_init(&s);
  fdt_sha256_append(&s, a, an);
  fdt_sha256_append(&s, b, bn);
  fdt_sha256_fini(&s, out);
}

/* fd_poh_mixin */
static inline void fdt_poh_mixin(uint8_t poh[32], const uint8_t mix[32]) { fdt_poh_sha2(poh, poh, 32, mix, 32); }

/* The root of cnt >= 1 signatures at arena + sig_offs[0 .. cnt): nodes is
   scratch of 32 cnt bytes.  Each layer is folded in place in ascending order;
   a last node without a partner is paired with itself. */
static inline void fdt_poh_sig_root(uint8_t root[32], const uint8_t *arena, const uint32_t *sig_offs, uint64_t cnt,
                                    uint8_t *nodes) {
  static const uint8_t LEAF = 0, BRANCH = 1;
  for (uint64_t j = 0; j < cnt; j++) {
    uint8_t m[65];
    m[0] = LEAF;
    memcpy(m + 1, arena + sig_offs[j], 64);
    fdt_poh_sha2(nodes + 32 * j, m, 65, m, 0);
  }
  for (uint64_t c = cnt; c > 1; c = (c + 1) / 2)
    for (uint64_t j = 0; j < (c + 1) / 2; j++) {
      uint8_t m[65];
      const uint64_t r = 2 * j + 1 < c ? 2 * j + 1 : c - 1;
      m[0] = BRANCH;
      memcpy(m + 1, nodes + 64 * j, 32);
      memcpy(m + 33, nodes + 32 * r, 32);
      fdt_poh_sha2(nodes + 32 * j, m, 65, m, 0);
    }
  memcpy(root, nodes, 32);
}

/* One entry whose arguments passed fdt_poh_args: out = its hash (zeros when
   too long); returns its code.  nodes: scratch of 32 * e->sig_cnt bytes. */
static inline int fdt_poh_entry(const uint8_t *arena, const fdgpu_poh_entry_t *e, const uint32_t *sig_offs, uint64_t cap,
                                uint8_t *nodes, uint8_t out[32]) {
  if (e->hash_cnt > cap) { memset(out, 0, 32); return FDGPU_CODE_POH_TOO_LONG; }
  memcpy(out, arena + e->prev_off, 32);
  fdt_poh_append(out, fdt_poh_chain_len(e));
  if (e->sig_cnt) {
    uint8_t root[32];
    fdt_poh_sig_root(root, arena, sig_offs + e->sig_first, e->sig_cnt, nodes);
    fdt_poh_mixin(out, root);
  } else if (e->mix_off != FDGPU_POH_NO_MIX) {
    fdt_poh_mixin(out, arena + e->mix_off);
  }
  return memcmp(out, arena + e->hash_off, 32) ? FDGPU_CODE_POH_MISMATCH : 0;
}
