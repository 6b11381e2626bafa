/* fdgpu_internal.h -- declarations shared by the kernel units (fdgpu_bcomb,
   fdgpu_verify, fdgpu_ingest, fdgpu_test_kernels, fdgpu_poh .hip) and the host engine
   (fdgpu_engine.h).  Not part of the public C ABI. */
#pragma once

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/fd_ed25519_gpu.h"
#include "../../include/fd_poh_gpu.h"

/* Per-signature work item (16 B, one dwordx4 per lane).  Offsets index the
   batch arena; the arena carries FDGPU_ARENA_SLACK readable bytes after
   the last payload byte. */
typedef struct {
  uint32_t msg_off;
  uint32_t msg_sz;
  uint32_t sig_off;   /* 64-B signature R || S */
  uint32_t pub_off;   /* 32-B public key */
} fdgpu_sig_desc_t;

/* Per-transaction combine item: signatures sig0 .. sig0+sig_cnt-1 of the
   signature array (batch_single_msg order).  sig_cnt outside [1,16] means
   the batch is rejected without verification (fd_ed25519_user.c:238-241). */
typedef struct {
  uint32_t sig0;
  uint32_t sig_cnt;
} fdgpu_txn_desc_t;

#define FDGPU_ARENA_SLACK   160u          /* readable bytes past the arena (SHA block loads) */
/* k in signed radix 16: 64 windows over the per-lane table {O, -A, .., -8A} */
#define FDGPU_ATAB_ENTRIES  9u            /* 0 (identity), 1A .. 8A (A negated) */
#ifndef FDGPU_ATAB_WORDS
#define FDGPU_ATAB_WORDS    40u           /* u32 per cached entry, unpacked (4 coordinates x 10 limbs) */
#endif
#define FDGPU_PTAB_WORDS    32u           /* u32 per stored table entry: 4 coordinates packed to 8 words, one 128-B line
                                             (fdgpu_atab.h) */
#ifndef FDGPU_VERIFY_WAVES
#define FDGPU_VERIFY_WAVES  2             /* waves per SIMD of the verify kernel: decode/pow chains want ~190 VGPRs */
#endif
#ifndef FDGPU_PHASE_STAMPS
#define FDGPU_PHASE_STAMPS  0             /* 1: per-phase cycle stamps (fdgpu_stamps.h), a diagnostic build */
#endif
/* Build switches: FDGPU_VERIFY_WAVES, FDGPU_ATAB_WORDS and FDGPU_PHASE_STAMPS,
   their defaults stated here once for every unit.  The shipped library is
   built with every one at its default;
   fdgpu_build_info() reports them and smoke() / bench.py refuse a library
   built otherwise (unless told it is an A/B build).  The slot-indexed
   workspace pool and the table store / load cache-policy switches were
   removed after their negative results (commit a5516cc is the
   last that holds them). */
/* Fixed-base comb for [S]B: S in signed radix 2^W, digit i looked up in
   table i = {0, 1, .., 2^(W-1)} x 2^(W i) B (affine niels, one 128-B line per
   entry), so [S]B costs NDIG mixed additions and no doublings.  Tables live
   in HBM (W=16: 16 x 32769 x 128 B = 67 MB, resident in the 256 MB Infinity
   Cache). */
#define FDGPU_BCOMB_BITS    16u           /* comb radix: NDIG tables of 2^(W-1)+1 entries */
#define FDGPU_BCOMB_NDIG    ((254u + FDGPU_BCOMB_BITS - 1u) / FDGPU_BCOMB_BITS)   /* covers S < 2^253 + carry */
#define FDGPU_BCOMB_ENTRIES ((1u << (FDGPU_BCOMB_BITS - 1u)) + 1u)
#define FDGPU_BCOMB_STRIDE  32u           /* u32 per entry (30 used): one 128-B line */
#define FDGPU_BCOMB_CHUNK   64u           /* entries per lane in the table build (one batch inversion) */
/* The verify equation with half-size scalars (fdgpu_lattice.h). */
#define HS_MAX_WIN          40u           /* radix-16 windows of |u|, |v| (< 2^159) */
/* A table's identity entry (digit 0) is one shared constant (g_tab_ident),
   so a lane stores entries 1..8 of each table */
#define FDGPU_TAB_STORED    (FDGPU_ATAB_ENTRIES - 1u)
/* The workspace holds FDGPU_WS_LANE_WORDS per lane (the size of 18 unpacked
   entries, kept: fdgpu_ws_bytes is part of the ABI), laid out as two regions:
     tables   lane i at word i * FDGPU_WS_TAB_WORDS: 16 packed entries, one
              128-B line each (2 KiB, line-aligned) -- entries 0..7 are 1..8
              of the -A table, 8..15 are 1..8 of the -R table;
     aux      after every lane's tables, FDGPU_WS_AUX_WORDS per lane, counted
              back from the region's end (where the fallback queue starts):
              lane i at end - (i + 1) * FDGPU_WS_AUX_WORDS.  Plain words: the
              park entry (k digits, code: the full path) at FDGPU_AUX_PARK and
              [w]B (or [S]B), an unpacked cached entry in canonical order, at
              FDGPU_AUX_SB; the rest of a lane's aux words is unused. */
#define FDGPU_WS_RTAB       FDGPU_TAB_STORED
#define FDGPU_WS_ENTRIES    (2u * FDGPU_TAB_STORED + 2u)                  /* 16 table entries, park, [w]B */
#define FDGPU_WS_LANE_WORDS (FDGPU_WS_ENTRIES * FDGPU_ATAB_WORDS)         /* 720 */
#define FDGPU_WS_TAB_WORDS  (2u * FDGPU_TAB_STORED * FDGPU_PTAB_WORDS)    /* 512 */
#define FDGPU_WS_AUX_WORDS  (FDGPU_WS_LANE_WORDS - FDGPU_WS_TAB_WORDS)    /* 208 */
#define FDGPU_AUX_PARK      0u
#define FDGPU_AUX_SB        FDGPU_ATAB_WORDS
#define FDGPU_BLOCK         256u
#define FDGPU_FLAG_REF_MAP  1u            /* portable-backend error mapping */
#define FDGPU_FLAG_KFULL    2u            /* half-size path: every lane takes the full-length fallback */
#define FDGPU_FLAG_KCACHE   4u            /* half-size path: one -A decode + table per distinct key */
#define FDGPU_FLAG_KPAIR    8u            /* half-size path, two lanes per signature (fdgpu_verify_pair_kernel) */
#define FDGPU_FLAG_KSPREAD  16u           /* one verify block per CU: dynamic LDS that leaves no room for a second */
/* The chain's LDS staging: one packed entry per lane and table, 8 chunks of
   16 B x 64 lanes per wave.  The verify block stages two entries a window
   (64 KB), the two-lane block one (32 KB).  FDGPU_FLAG_KSPREAD adds the
   dynamic LDS that brings a block to just over half of a CU's 160 KB, so a
   second block does not fit. */
#define FDGPU_STAGE_WAVE_WORDS (FDGPU_PTAB_WORDS / 4u * 256u)
#define FDGPU_STAGE_LDS        (FDGPU_BLOCK / 64u * 2u * FDGPU_STAGE_WAVE_WORDS * 4u)
#define FDGPU_STAGE_LDS_PAIR   (FDGPU_BLOCK / 64u * FDGPU_STAGE_WAVE_WORDS * 4u)
#define FDGPU_CU_LDS           (160u * 1024u)
#define FDGPU_SPREAD_LDS       (FDGPU_CU_LDS / 2u - FDGPU_STAGE_LDS + 1024u)
#define FDGPU_SPREAD_LDS_PAIR  (FDGPU_CU_LDS / 2u - FDGPU_STAGE_LDS_PAIR + 1024u)
#ifdef __cplusplus
static_assert(2u * (FDGPU_STAGE_LDS + FDGPU_SPREAD_LDS) > FDGPU_CU_LDS &&
              2u * (FDGPU_STAGE_LDS_PAIR + FDGPU_SPREAD_LDS_PAIR) > FDGPU_CU_LDS &&
              FDGPU_STAGE_LDS + FDGPU_SPREAD_LDS <= FDGPU_CU_LDS && FDGPU_STAGE_LDS_PAIR + FDGPU_SPREAD_LDS_PAIR <= FDGPU_CU_LDS,
              "a spread launch's LDS admits one block per CU, and no more");
#endif
/* The verify blocks (two 256-VGPR waves per SIMD) fill every SIMD's register
   file, so a kernel queued behind or beside a running verify starts its
   workgroups only as verify blocks retire: a launch of many workgroups then
   waits through many retirements before its last one runs (rocprofv3, host-fed
   1M batches: an empty fallback launch of 512 blocks took 0.8 ms, the 3,907-
   block combine 0.66 ms; profiles/r05/hostfed_trace.md).  The short kernels
   around the verify therefore run on few, fat workgroups that stride over
   their work: */
#define FDGPU_FULL_BLOCKS   16u           /* the fallback chain: its queue is ~empty (split failures ~2^-30) */
#define FDGPU_AUX_BLOCKS    64u           /* combine */
/* The gathered batches' ingest and finish: a workgroup resident beside the
   verify holds a verify block's slot on its CU for its whole life (its waves
   take VGPRs the second verify wave needs), and these kernels wait on the bus,
   so their slot time -- not their own duration -- is what the verify loses.
   16 blocks that each keep more bus accesses in flight cost a quarter of the
   slot time of 64 and still fill PCIe (profiles/r05/ubench_pcie.jsonl: 16 x
   256 threads read 57 GB/s): engine-only gathered capacity, two engines,
   69 -> 81 M txn/s, and two cfg1 tiles 58.8 -> 71.5 M
   (profiles/r05/aux_blocks.md).  FDGPU_AUX_BLOCKS_IN / _FIN override. */
#define FDGPU_IO_BLOCKS     16u
/* SHA-512 block-count groups of the host-side bucketing (expand): messages of
   more blocks than this share the last group */
#define FDGPU_NBLK_GROUPS   32u
/* PoH chains (fdgpu_poh.hip): hashes a lane runs between two looks at the entry
   queue.  64 hashes are ~10^5 instructions, against which the ballot and the
   finished lanes' mixin and stores are noise; a finished lane idles for at
   most this many hashes of its wave */
#define FDGPU_POH_CHUNK     64u

#ifdef __cplusplus
extern "C" {
#endif

/* Launchers, under the unit that defines each with its kernels; all
   asynchronous on `stream` unless noted */

/* ---- fdgpu_bcomb.hip ---- */
size_t     fdgpu_btab_bytes(void);                                   /* fixed-base table size */
/* builds the fixed-base table into d_btab (fdgpu_btab_bytes()); synchronous */
hipError_t fdgpu_btab_build(uint32_t *d_btab, hipStream_t stream);

/* ---- fdgpu_verify.hip ---- */
/* one signature per lane; d_ws must hold fdgpu_ws_bytes(n_sig) bytes */
/* d_perm (NULL = identity): d_sig_codes[d_perm[i]] receives the code of
   descriptor i (descriptors grouped by SHA-512 block count, codes in the
   caller's order) */
/* d_n_sig != NULL: the signature count is read on the device (it is produced
   there by the GPU-side ingest); n_sig is then an upper bound that sizes the
   grid (and the workspace).  resident_blocks: verify-kernel blocks the
   device keeps resident (occupancy x CUs, the fallback kernel's grid cap);
   kc_seed: the key cache's hash seed (FDGPU_FLAG_KCACHE). */
hipError_t fdgpu_launch_verify_sigs(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_sigs, uint32_t n_sig,
                                    const uint32_t *d_perm, const uint32_t *d_btab, uint32_t *d_ws,
                                    int8_t *d_sig_codes, uint32_t flags, hipStream_t stream,
                                    const uint32_t *d_n_sig, uint32_t resident_blocks, uint64_t kc_seed,
                                    int cnt_zeroed = 0);
/* The synchronous API's messages too large for one arena: SHA-512(R_i ||
   A_i || M) of n <= 64 signatures over one message, a piece of M per launch
   (blocks [blk0, blk0 + nblk) of fdgpu_sha512_stream_blocks(msg_sz); d_mbuf
   = M[m0, m0 + mlen) covering those blocks' message bytes; d_ra = n x (R ||
   A); d_state = n x 8 words), then the verify from those states
   (descriptor i: msg_off = the offset of state i in d_arena, 8-B aligned;
   of flags FDGPU_FLAG_REF_MAP, FDGPU_FLAG_KFULL and FDGPU_FLAG_KPAIR are
   read, the last two for the chain diagnostic). */
uint64_t   fdgpu_sha512_stream_blocks(uint64_t msg_sz);
hipError_t fdgpu_launch_sha512_stream(const uint8_t *d_mbuf, uint64_t m0, uint64_t mlen, uint64_t msg_sz,
                                      uint64_t blk0, uint32_t nblk, const uint8_t *d_ra, uint64_t *d_state,
                                      uint32_t n, hipStream_t stream);
hipError_t fdgpu_launch_verify_prehashed(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_sigs, uint32_t n_sig,
                                         const uint32_t *d_btab, uint32_t *d_ws, int8_t *d_sig_codes, uint32_t flags,
                                         hipStream_t stream);
/* The verify workspace of an n_sig batch, in u32 words from d_ws (128-B
   aligned): the lanes' words (FDGPU_WS_LANE_WORDS each, lanes = n_sig rounded
   up to whole blocks: every lane's packed tables, FDGPU_WS_TAB_WORDS each,
   then the lanes' aux words, which end where the queue starts -- the kernels
   find a lane's aux words from the queue's address),
   the fallback queue (one word per lane), 16 words of counters (the queue's
   count, then the key cache's representative count), the key cache's hash
   table (ht_slots, a power of two >= 2 lanes and >= 64), then key_of,
   verdicts and representatives (one word per lane each).  A caller whose
   earlier kernel on the stream zeroes *cnt passes cnt_zeroed to
   fdgpu_launch_verify_sigs (no memset). */
typedef struct {
  uint64_t lanes, ht_slots;
  uint32_t *queue, *cnt, *rep_cnt, *ht, *key_of, *kverd, *reps;
  size_t bytes;
} fdgpu_ws_layout_t;
static inline fdgpu_ws_layout_t fdgpu_ws_layout(uint32_t *d_ws, uint64_t n_sig) {
  fdgpu_ws_layout_t l;
  l.lanes = (n_sig + FDGPU_BLOCK - 1) / FDGPU_BLOCK * FDGPU_BLOCK;
  for (l.ht_slots = 64; l.ht_slots < 2 * l.lanes;) l.ht_slots <<= 1;
  const uint64_t queue = l.lanes * FDGPU_WS_LANE_WORDS, cnt = queue + l.lanes, ht = cnt + 16, key_of = ht + l.ht_slots;
  auto at = [d_ws](uint64_t word) { return d_ws ? d_ws + word : nullptr; };   /* NULL: only the sizes are wanted */
  l.queue = at(queue);
  l.cnt = at(cnt);
  l.rep_cnt = at(cnt + 1);
  l.ht = at(ht);
  l.key_of = at(key_of);
  l.kverd = at(key_of + l.lanes);
  l.reps = at(key_of + 2 * l.lanes);
  l.bytes = (size_t)(key_of + 3 * l.lanes) * sizeof(uint32_t);
  return l;
}
/* One batch of a merged verify launch (FDGPU_FLAG_MERGE): what
   fdgpu_launch_verify_sigs takes per batch, read by each block from a table
   in pinned host memory (blockIdx.y picks the batch). */
typedef struct {
  const uint8_t *arena;
  const fdgpu_sig_desc_t *sigs;
  const uint32_t *n_sig;       /* the count, produced on the device (parse + expand) */
  uint32_t *ws;                /* the batch's workspace; its fallback queue and counter follow the lanes */
  int8_t *codes;
  uint32_t *queue, *cnt;
  uint32_t bound;              /* the launch bound of the count: the batch's blocks */
  uint32_t slow;               /* fallback blocks */
} fdgpu_mbatch_t;
/* one verify (one lane per signature) + one fallback launch over nb batches:
   grids {max blocks, nb} */
hipError_t fdgpu_launch_verify_multi(const fdgpu_mbatch_t *mb, uint32_t nb, uint32_t grid_max, uint32_t slow_max,
                                     const uint32_t *d_btab, uint32_t flags, hipStream_t stream);
/* d_accept (NULL: not written): ceil(n_txn / 64) words, bit t = txn t verified */
hipError_t fdgpu_launch_combine(const fdgpu_txn_desc_t *d_txns, uint32_t n_txn, const int8_t *d_sig_codes,
                                int8_t *d_txn_codes, uint64_t *d_accept, hipStream_t stream);
hipError_t fdgpu_verify_occupancy(int *blocks_per_cu);
/* the kernels' compile-time switches as JSON members into buf; 1 iff all are
   at the shipped defaults */
int        fdgpu_kernel_build_info(char *buf, size_t n);
size_t     fdgpu_ws_bytes(uint64_t n_sig);

/* ---- fdgpu_ingest.hip ---- */
/* loads the unit's code object (engine open: before the first frag batch) */
__attribute__((visibility("hidden"))) hipError_t fdgpu_ingest_load(void);
/* GPU-side ingest: parse n raw payloads (frags index d_arena), scan the
   signature counts, expand the descriptors; the batch's signature count is
   left in *d_n_sig.  Buffers: d_txn_out n x FDT_TXN_MAX_SZ, d_txn_sz /
   d_txd / d_cnt / d_sig0 / d_tds n entries, d_blocktot ceil(n / 1024),
   d_sigs the sum of fdgpu_frag_sig_bound over the frags. */
uint64_t   fdgpu_frag_sig_bound(uint32_t sz);
/* d_frags: n records of frag_stride u32 words whose first two are {off, sz}
   (fdgpu_frag_t: 2, fdgpu_frag_ex_t: 4) */
hipError_t fdgpu_launch_frag_ingest(const uint8_t *d_arena, const void *d_frags, uint32_t frag_stride, uint32_t n,
                                    uint8_t *d_txn_out, uint16_t *d_txn_sz, fdgpu_txn_t *d_txd, uint32_t *d_cnt,
                                    uint32_t *d_sig0, uint32_t *d_blocktot, uint32_t *d_n_sig,
                                    fdgpu_sig_desc_t *d_sigs, fdgpu_txn_desc_t *d_tds, hipStream_t stream);
hipError_t fdgpu_launch_frag_codes(const uint16_t *d_txn_sz, uint32_t n, int8_t *d_codes, hipStream_t stream);
/* fdgpu_submit_frags, in two launches for batches up to FDGPU_SMALL_SCAN_MAX
   txns (parse, then scan + expand in one block; larger batches take
   fdgpu_launch_frag_ingest's path), and the batch's end in one launch
   (combine + parse failures + trailer pack; codes at d_codes, trailers at
   d_trailers). */
#define FDGPU_SMALL_SCAN_MAX 65536u
hipError_t fdgpu_launch_frag_ring(const uint8_t *d_arena, const fdgpu_frag_ex_t *d_fx, uint32_t n, uint8_t *d_txn_out,
                                  uint16_t *d_txn_sz, fdgpu_txn_t *d_txd, uint32_t *d_cnt, uint32_t *d_sig0,
                                  uint32_t *d_blocktot, uint32_t *d_n_sig, fdgpu_sig_desc_t *d_sigs,
                                  fdgpu_txn_desc_t *d_tds, hipStream_t stream);
hipError_t fdgpu_launch_frag_finish(const fdgpu_txn_desc_t *d_tds, uint32_t n, const int8_t *d_sig_codes,
                                    const uint16_t *d_txn_sz, const fdgpu_frag_ex_t *d_fx, const uint8_t *d_txn_out,
                                    int8_t *d_codes, uint8_t *d_trailers, hipStream_t stream);
/* fdgpu_submit_frags_io's kernels, each on at most FDGPU_IO_BLOCKS blocks
   whose waves stride over groups of 64 frags.  Ingest: per group, the wave
   reads the 64 records and payload addresses (one coalesced read of each over
   the bus), copies the group's payloads (16-B units, flattened over the
   group, four loads in flight per lane) from host memory (d_src[i], the
   registered region's device-side address) to d_arena + d_fx[i].off; with
   d_chk (n pairs {mcache line address, seq}, line 0: none) each line is
   re-read once the payload loads have returned, and a republished one marks
   the kept record FDGPU_FX_LAPPED; then lane i parses frag i (fd_txn_parse)
   and the wave takes its descriptor slots with one atomic add on *d_n_sig,
   which must be zero at the start (the finish kernel of the slot's previous
   gathered batch clears it: d_zero_next).  Finish: per group, lane i writes
   frag i's code, dedup tag and out size, then the wave assembles the group's
   out frags at d_out + d_fx[i].tr_off ([payload][pad][fd_txn_t][u16 sz]) in
   16-B stores. */
#define FDGPU_FX_LAPPED 0x80000000u     /* in fdgpu_frag_ex_t.tr_cap (out_cap <= 0xFFFF) */
/* DMA gather (d_rtab != NULL): the payloads already lie in the batch arena
   (the DMA engines copied the batch's source ranges there); a record's sz
   carries its range (bits 16..23) and off its offset in that range, and the
   ingest kernel only resolves off = d_rtab[range] + off */
#define FDGPU_IO_RANGES_MAX 255u
uint64_t   fdgpu_frag_fp_bound(uint32_t sz);
hipError_t fdgpu_launch_frag_ingest_io(const uint64_t *d_src, const fdgpu_frag_ex_t *d_fx, const uint64_t *d_chk,
                                       const uint64_t *d_rtab, uint32_t n, uint8_t *d_arena,
                                       fdgpu_frag_ex_t *d_fx_dev, uint8_t *d_txn_out, uint16_t *d_txn_sz,
                                       fdgpu_sig_desc_t *d_sigs, fdgpu_txn_desc_t *d_tds, uint32_t *d_n_sig,
                                       uint32_t *d_zero_word, hipStream_t stream);
hipError_t fdgpu_launch_frag_finish_io(const fdgpu_txn_desc_t *d_tds, uint32_t n, const int8_t *d_sig_codes,
                                       const uint16_t *d_txn_sz, const fdgpu_frag_ex_t *d_fx, const uint8_t *d_txn_out,
                                       const uint8_t *d_arena, uint64_t hash_seed, uint8_t *d_out, int8_t *d_codes,
                                       uint64_t *d_tags, uint16_t *d_out_szs, uint32_t *d_zero_next,
                                       hipStream_t stream);

/* ---- fdgpu_poh.hip (the shred unit's launchers: fdgpu_shred.h) ---- */
/* Leaves and roots of a PoH batch: d_nodes (8 u32 a node, 16-B aligned, one
   per signature) receives SHA-256(0x00 || arena[d_sig_offs[j], +64)) as
   big-endian words, then each entry's range is folded in place and its root
   left in node sig_first.  Reads up to 16 bytes past a signature (the arena's
   slack). */
hipError_t fdgpu_launch_poh_tree(const uint8_t *d_arena, const fdgpu_poh_entry_t *d_entries, uint32_t n,
                                 const uint32_t *d_sig_offs, uint32_t sig_total, uint32_t *d_nodes, hipStream_t stream);
/* The chains, after the tree on the same stream: d_order[0, n_q) are the
   entries with hash_cnt <= cap, longest first; *d_head (cleared here, on the
   stream) is the queue's head.  grid_waves: the grid in waves (0: one per 64
   entries, at most four per SIMD).  d_codes[i] and d_hashes + 32 i (16-B
   aligned) for every entry, those above the cap included. */
hipError_t fdgpu_launch_poh_chains(const uint8_t *d_arena, const fdgpu_poh_entry_t *d_entries, uint32_t n,
                                   const uint32_t *d_order, uint32_t n_q, const uint32_t *d_nodes, uint32_t cap,
                                   uint32_t grid_waves, uint32_t *d_head, int8_t *d_codes, uint8_t *d_hashes,
                                   hipStream_t stream);

/* ---- fdgpu_test_kernels.hip: per-stage diagnostics ---- */
hipError_t fdgpu_launch_test_fe(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream);
hipError_t fdgpu_launch_test_decode(const uint32_t *d_enc, uint32_t *d_out, uint32_t n, uint32_t flags, hipStream_t stream);
hipError_t fdgpu_launch_test_sha512(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_msgs, uint32_t n,
                                    uint32_t *d_out, hipStream_t stream);
hipError_t fdgpu_launch_test_hram(const uint8_t *d_arena, const fdgpu_sig_desc_t *d_sigs, uint32_t n,
                                  uint32_t *d_out, hipStream_t stream);
hipError_t fdgpu_launch_test_sc_reduce(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream);
hipError_t fdgpu_launch_test_hs_split(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream);
/* the group layer (tests/test_gpu_group.py): field ops on raw limbs (20 u32 in, 80 out), every group
   operation on a pair of points (fdgpu_test_ge_in_words() in, 32 x fdgpu_test_ge_results() out), and the
   two scalar recodings (8 in, 16 out) */
hipError_t fdgpu_launch_test_fe_raw(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream);
uint32_t   fdgpu_test_ge_in_words(void);
uint32_t   fdgpu_test_ge_results(void);
hipError_t fdgpu_launch_test_ge(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream);
hipError_t fdgpu_launch_test_sc_recode(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream);
/* the packed table entry (tests/test_gpu_tabpack.py): a cached entry's 40 raw limbs in; per record
   FDGPU_TABPACK_OUT_WORDS out (a multiple of a line: d_out must be 128-B aligned) -- the 32 words
   atab_store leaves, then the 40 limbs of atab_load, of stage_entry + unstage_entry_signed, and of the
   same with neg */
#define FDGPU_TABPACK_OUT_WORDS 160u
hipError_t fdgpu_launch_test_tabpack(const uint32_t *d_in, uint32_t *d_out, uint32_t n, hipStream_t stream);

/* ---- fdgpu_diag.cpp: the group layer's diagnostics, exported for the parity tests beside the
   fdgpu_debug_* of include/fd_ed25519_gpu.h (same conventions: synchronous, 0 on success) ---- */
int      fdgpu_debug_fe_raw(fdgpu_engine_t *e, uint8_t const *fg, uint64_t n, uint8_t *out);
int      fdgpu_debug_ge_ops(fdgpu_engine_t *e, uint8_t const *in, uint64_t n, uint8_t *out);
int      fdgpu_debug_sc_recode(fdgpu_engine_t *e, uint8_t const *s, uint64_t n, uint8_t *out);
/* n cached entries (40 u32 raw limbs each: Y+X, Y-X, 2Z, 2dT) through the table's store, load and LDS
   path; FDGPU_TABPACK_OUT_WORDS u32 per entry out */
int      fdgpu_debug_tabpack(fdgpu_engine_t *e, uint8_t const *in, uint64_t n, uint8_t *out);
/* the verify chain at chosen k (tests/test_gpu_chain.py): n descriptors whose msg_off is the offset (8-B
   aligned) of 64 B of SHA-512 state words in the arena, as the synchronous API's over-arena path lays them
   out, through fdgpu_launch_verify_prehashed with a workspace of its own; flags of FDGPU_FLAG_REF_MAP,
   FDGPU_FLAG_KFULL (every lane queued) and FDGPU_FLAG_KPAIR (the two-lane kernel).  Descriptor i is lane i.
   codes_out: n codes; *n_full_out: the fallback queue's count once the stream has drained */
int      fdgpu_debug_verify_prehashed(fdgpu_engine_t *e, uint8_t const *arena, uint64_t arena_sz,
                                      fdgpu_sig_desc_t const *descs, uint64_t n, uint32_t flags, int8_t *codes_out,
                                      uint32_t *n_full_out);
/* n_entries x FDGPU_BCOMB_STRIDE words of the engine's fixed-base table, from entry first_entry of the
   flat (table, entry) order, to the host; no kernel runs */
int      fdgpu_debug_btab(fdgpu_engine_t *e, uint64_t first_entry, uint64_t n_entries, uint32_t *out);
/* the comb's shape: which = 0 W, 1 NDIG, 2 entries per table, 3 words per entry, 4 entries per fill chunk */
uint32_t fdgpu_bcomb_dim(int which);

#ifdef __cplusplus
}
#endif
