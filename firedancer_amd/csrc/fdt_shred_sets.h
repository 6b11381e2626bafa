/* fdt_shred_sets.h -- the rule of a set batch (include/fd_shred_sets_gpu.h) on the host, after the roots: the
   argument check, each shred's state, the grouping of the shreds without a known root by their 128 key bytes, and
   the scatter of the groups' codes.  One source for the host library (tile/fdt_callers.cpp: fdgpu_shred_sets_verify)
   and the sanitizer program (tools/shred_sets_san.cpp).  Host only. */
#pragma once

#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/fd_shred_sets_gpu.h"

/* every shred, leader key and known root inside the arena: 1, else 0 */
static inline int fdt_shred_sets_args(uint64_t arena_sz, const fdgpu_set_shred_t *shreds, uint64_t n) {
  if (n >= UINT32_MAX) return 0;
  for (uint64_t i = 0; i < n; i++)
    if ((uint64_t)shreds[i].off + shreds[i].sz > arena_sz || (uint64_t)shreds[i].pub_off + 32 > arena_sz ||
        (shreds[i].known_off != FDGPU_SHRED_NO_ROOT && (uint64_t)shreds[i].known_off + 32 > arena_sz))
      return 0;
  return 1;
}

/* ok[i]: shred i passed fdt_shred_check_core, its root at roots + 32 i.  Writes the codes of the shreds that need no
   verify (rejected: FDGPU_CODE_SHRED_REJECT; known root: 0 or FDGPU_CODE_SHRED_ROOT_MISMATCH) and rep[i] = UINT32_MAX
   for them; for every other shred rep[i] = the first shred with its key (signature 64, root 32, leader key 32).
   reps: those first shreds, ascending. */
static inline void fdt_shred_sets_group(const uint8_t *arena, const fdgpu_set_shred_t *shreds, uint64_t n, const uint8_t *ok,
                                        const uint8_t *roots, int8_t *codes, uint32_t *rep, std::vector<uint32_t> &reps) {
  std::unordered_map<std::string, uint32_t> first;
  std::string key(128, '\0');
  reps.clear();
  for (uint64_t i = 0; i < n; i++) {
    rep[i] = UINT32_MAX;
    if (!ok[i]) { codes[i] = FDGPU_CODE_SHRED_REJECT; continue; }
    if (shreds[i].known_off != FDGPU_SHRED_NO_ROOT) {
      codes[i] = memcmp(roots + 32 * i, arena + shreds[i].known_off, 32) ? FDGPU_CODE_SHRED_ROOT_MISMATCH : 0;
      continue;
    }
    memcpy(&key[0], arena + shreds[i].off, 64);
    memcpy(&key[64], roots + 32 * i, 32);
    memcpy(&key[96], arena + shreds[i].pub_off, 32);
    const auto it = first.emplace(key, (uint32_t)i);
    rep[i] = it.first->second;
    if (it.second) reps.push_back((uint32_t)i);
  }
}

/* rep_codes[k]: the verify's code of shred reps[k].  A group's code is its representative's; reps ascends, so a
   representative's place in it is found by search. */
static inline void fdt_shred_sets_scatter(uint64_t n, const uint32_t *rep, const std::vector<uint32_t> &reps,
                                          const int8_t *rep_codes, int8_t *codes) {
  for (uint64_t i = 0; i < n; i++)
    if (rep[i] != UINT32_MAX)
      codes[i] = rep_codes[(size_t)(std::lower_bound(reps.begin(), reps.end(), rep[i]) - reps.begin())];
}
