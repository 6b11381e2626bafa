/* fdt_shred.h -- the shred rules as one source for the host and the GPU:
   what the shred tile checks of a shred before it trusts it, up to the
   Merkle root its leader signed.

   fdt_shred_check_core restates, in the reference's order,
     fd_shred_parse            src/ballet/shred/fd_shred.c:3-72
     fd_fec_resolver_add_shred src/disco/shred/fd_fec_resolver.c:336-393
                               (the checks before the signature)
   and fdt_shred_root_core the leaf hash and the walk up the inclusion proof
     fd_bmtree_hash_leaf       src/ballet/bmtree/fd_bmtree.c:50-68
     fd_bmtree_from_proof      fd_bmtree.c:350-378 (what
                               fd_bmtree_commitp_insert_with_proof does on
                               an empty tree, fd_fec_resolver.c:430).
   Quirks are restated, not fixed: see the comments at each.

   Compiled by g++ into libfd_verify_tile.so (fdt_shred_check,
   fdt_shred_root with the scalar fdt_sha256.h) and by hipcc into
   fdgpu_shred_ingest_kernel (one shred per lane; the hashes there are
   fdgpu_sha256.h's), so both sides apply the same rules.

   Field offsets in the shred (fd_shred.h:150-226, packed little-endian):
     signature 0x00 (64 B)   variant 0x40   slot 0x41   idx 0x49
     version 0x4d   fec_set_idx 0x4f   data.size 0x56
     code.data_cnt 0x53   code.code_cnt 0x55   code.idx 0x57 */
#pragma once

#include <stdint.h>

#include "fdt_parse.h"
#if !defined(__HIP_DEVICE_COMPILE__)
#include "fdt_sha256.h"
#endif

#define FDT_SHRED_MIN_SZ         1203u     /* FD_SHRED_MIN_SZ (fd_shred.h:87): a data shred */
#define FDT_SHRED_MAX_SZ         1228u     /* FD_SHRED_MAX_SZ (fd_shred.h:83): a code shred */
#define FDT_SHRED_DATA_HEADER_SZ 0x58u
#define FDT_SHRED_CODE_HEADER_SZ 0x59u
#define FDT_SHRED_NODE_SZ        20u       /* FD_SHRED_MERKLE_NODE_SZ */
#define FDT_SHRED_ROOT_SZ        32u       /* FD_SHRED_MERKLE_ROOT_SZ */
#define FDT_SHRED_SIG_SZ         64u
#define FDT_SHRED_IN_TYPE_MAX    67u       /* FD_REEDSOL_DATA_SHREDS_MAX == FD_REEDSOL_PARITY_SHREDS_MAX */
#define FDT_SHRED_DEPTH_MAX      9u        /* INCLUSION_PROOF_LAYERS - 1 (fd_fec_resolver.c:9) */
#define FDT_BMTREE_PREFIX_SZ     26u       /* FD_BMTREE_LONG_PREFIX_SZ */
/* fd_bmtree_leaf_prefix / fd_bmtree_node_prefix (fd_bmtree.c:30-31), the first 26 bytes */
#define FDT_BMTREE_LEAF_PREFIX   "\x00SOLANA_MERKLE_SHREDS_LEAF"
#define FDT_BMTREE_NODE_PREFIX   "\x01SOLANA_MERKLE_SHREDS_NODE"

/* fd_bmtree_depth (fd_bmtree.c:146-153): layers of a tree of leaf_cnt leaves */
FDT_HD uint32_t fdt_bmtree_depth(uint32_t leaf_cnt) {
  if (leaf_cnt <= 1u) return leaf_cnt;
  uint32_t msb = 0;
  for (uint32_t v = leaf_cnt - 1u; v >>= 1;) msb++;
  return msb + 2u;
}

/* 1 and *out filled if the shred passes every check before the signature, 0
   if the shred tile would drop it.  buf[0, sz) is untrusted; nothing past sz
   is used (on the GPU the reader's 16-B windows may touch the arena's slack,
   and what they hold there never reaches a decision: every field read lies
   below 0x58 <= sz). */
FDT_HD int fdt_shred_check_core(const uint8_t *buf, uint64_t sz, uint16_t expected_version, fdt_shred_chk_t *out) {
  fdt_reader r;
  r.p = buf; r.sz = sz; r.i = 0; r.fail = 0;
  /* ---- fd_shred_parse ---- */
  if (sz < FDT_SHRED_DATA_HEADER_SZ) return 0;                                   /* fd_shred.c:8 */
  const uint32_t variant = r.at(0x40), type = variant & 0xf0u;
  const bool six = type == 0x80u || type == 0x40u || type == 0x90u || type == 0x60u || type == 0xb0u || type == 0x70u;
  if (!six && variant != 0xa5u && variant != 0x5au) return 0;                    /* :16-24 */
  const bool legacy = type == 0xa0u || type == 0x50u;
  const bool chained = type == 0x90u || type == 0x60u || type == 0xb0u || type == 0x70u;
  const bool resigned = type == 0xb0u || type == 0x70u;
  const uint32_t depth = legacy ? 0u : (variant & 0xfu);                         /* fd_shred_merkle_cnt */
  const uint64_t proof_sz = (uint64_t)FDT_SHRED_NODE_SZ * depth, prev_root_sz = chained ? FDT_SHRED_ROOT_SZ : 0u;
  uint64_t need;
  if (type & 0x80u) {                                                            /* FD_SHRED_TYPEMASK_DATA, :41-59 */
    const uint64_t size = (uint64_t)r.at(0x56) | ((uint64_t)r.at(0x57) << 8);
    if (size < FDT_SHRED_DATA_HEADER_SZ) return 0;
    if (type != 0xa0u && sz < FDT_SHRED_MIN_SZ) return 0;
    /* `type & 0x20` is the reference's test for a legacy data shred (:55); the
       resigned data type 0xb0 has that bit too, so for it -- as for 0xa0 --
       the bound is the packet's size, not 1203 */
    const uint64_t effective = (type & 0x20u) ? sz : FDT_SHRED_MIN_SZ;
    if (effective < FDT_SHRED_DATA_HEADER_SZ + proof_sz + (size - FDT_SHRED_DATA_HEADER_SZ) + prev_root_sz) return 0;
    need = effective;                     /* header + payload + zero padding + proof + previous root */
  } else if (type & 0x40u) {                                                     /* FD_SHRED_TYPEMASK_CODE, :60-66 */
    if (FDT_SHRED_CODE_HEADER_SZ + prev_root_sz + proof_sz > FDT_SHRED_MAX_SZ) return 0;
    need = FDT_SHRED_MAX_SZ;
  } else {
    return 0;
  }
  if (sz < need) return 0;                                                       /* :69 */
  /* ---- fd_fec_resolver_add_shred, before the signature ---- */
  uint32_t any = 0;
  for (uint32_t k = 0; k < FDT_SHRED_SIG_SZ; k++) any |= r.at(k);
  if (!any) return 0;                                                            /* fd_fec_resolver.c:336 */
  if (legacy) return 0;                                                          /* :349-352 */
  const uint32_t version = (uint32_t)r.at(0x4d) | ((uint32_t)r.at(0x4e) << 8);
  if (version != expected_version) return 0;                                     /* :354 */
  const bool is_data = (type & 0xc0u) == 0x80u;
  uint32_t data_cnt = 0;
  if (!is_data) {                                                                /* :358-362 */
    data_cnt = (uint32_t)r.at(0x53) | ((uint32_t)r.at(0x54) << 8);
    const uint32_t code_cnt = (uint32_t)r.at(0x55) | ((uint32_t)r.at(0x56) << 8);
    if (data_cnt > FDT_SHRED_IN_TYPE_MAX || code_cnt > FDT_SHRED_IN_TYPE_MAX) return 0;
    if (!data_cnt || !code_cnt) return 0;
  }
  uint32_t in_type_idx;
  if (is_data) {                          /* idx - fec_set_idx in 32-bit unsigned arithmetic: it wraps (:384) */
    const uint32_t idx = (uint32_t)r.at(0x49) | ((uint32_t)r.at(0x4a) << 8) | ((uint32_t)r.at(0x4b) << 16) | ((uint32_t)r.at(0x4c) << 24);
    const uint32_t fec = (uint32_t)r.at(0x4f) | ((uint32_t)r.at(0x50) << 8) | ((uint32_t)r.at(0x51) << 16) | ((uint32_t)r.at(0x52) << 24);
    in_type_idx = idx - fec;
  } else {
    in_type_idx = (uint32_t)r.at(0x57) | ((uint32_t)r.at(0x58) << 8);            /* 0x58 < 1228 <= sz */
  }
  if (in_type_idx >= FDT_SHRED_IN_TYPE_MAX) return 0;                            /* :387 */
  const uint32_t shred_idx = is_data ? in_type_idx : in_type_idx + data_cnt;     /* :385 */
  if (depth > FDT_SHRED_DEPTH_MAX) return 0;                                     /* :392 */
  if (fdt_bmtree_depth(shred_idx + 1u) > depth + 1u) return 0;                   /* :393 */
  out->shred_idx = shred_idx;
  out->depth = depth;
  /* fd_shred_merkle_off (fd_shred.h:357-362); the leaf is everything between the signature and the proof
     (merkle_protected_sz, fd_fec_resolver.c:368-375) */
  out->proof_off = (is_data ? FDT_SHRED_MIN_SZ : FDT_SHRED_MAX_SZ) - FDT_SHRED_NODE_SZ * depth - (resigned ? FDT_SHRED_SIG_SZ : 0u);
  out->leaf_off = FDT_SHRED_SIG_SZ;
  out->leaf_end = out->proof_off;
  return 1;
}

#if !defined(__HIP_DEVICE_COMPILE__)
/* The Merkle root the leader signed, from a shred that passed fdt_shred_check_core
   (chk is its result): the leaf hash, then one node hash per proof layer, the
   proof's node on the right iff bit l of shred_idx is 0; nodes are the first
   20 bytes of a hash, the root is all 32 of the last one. */
static inline void fdt_shred_root_core(const uint8_t *buf, const fdt_shred_chk_t *chk, uint8_t root[32]) {
  fdt_sha256_t s;
  uint8_t cur[32];
  fdt_sha256_init(&s);
  fdt_sha256_append(&s, FDT_BMTREE_LEAF_PREFIX, FDT_BMTREE_PREFIX_SZ);
  fdt_sha256_append(&s, buf + chk->leaf_off, chk->leaf_end - chk->leaf_off);
  fdt_sha256_fini(&s, cur);
  for (uint32_t l = 0; l < chk->depth; l++) {
    const uint8_t *node = buf + chk->proof_off + FDT_SHRED_NODE_SZ * l;
    const bool cur_left = !((chk->shred_idx >> l) & 1u);
    fdt_sha256_init(&s);
    fdt_sha256_append(&s, FDT_BMTREE_NODE_PREFIX, FDT_BMTREE_PREFIX_SZ);
    fdt_sha256_append(&s, cur_left ? cur : node, FDT_SHRED_NODE_SZ);
    fdt_sha256_append(&s, cur_left ? node : cur, FDT_SHRED_NODE_SZ);
    fdt_sha256_fini(&s, cur);
  }
  memcpy(root, cur, 32);
}
#endif
