// Paged KV cache addressing (infer/cache.py PagedKVCache; decode.hip attn_decode_paged, rope.hip
// rope_kv_write_paged_).
//
// A layer's K and V are page pools [num_pages, page_size, Hkv, hd]; one int32 block table [B, NP],
// shared by every layer, maps logical row r of sequence b to pool row
//     bt[b, r >> lg] * page_size + (r & (page_size - 1)),        page_size = 1 << lg.
// Page 0 is the null page: the allocator never hands it out and every unassigned entry is 0, so any
// lookup inside the table stays inside the pool -- a write to an unreserved row lands in page 0, which
// nothing valid reads -- and the kernels need no branch for it. Rows outside [0, NP * page_size) are
// the caller's to drop BEFORE the lookup.
#pragma once
#include "spa_debug.h"

namespace spa {

struct PagedTable {
  const int* bt;  // [B, NP] int32, contiguous
  int NP, lg, num_pages;
};

// page id of logical row `row` (inside [0, NP * page_size)) of sequence b. Debug-bounds build: the
// table index and the page id are guarded, and a bad id reads the null page instead.
__device__ __forceinline__ int paged_page(const PagedTable& tb, int b, long row) {
  const long e = row >> tb.lg;
  SPA_DBG_CHECK(e, tb.NP);
  int page = tb.bt[(long)b * tb.NP + e];
  if (!SPA_DBG_OK(page, tb.num_pages)) page = 0;
  return page;
}

// pool row of logical row `row` in page `page`
__device__ __forceinline__ long paged_pool_row(const PagedTable& tb, int page, long row) {
  return ((long)page << tb.lg) + (row & ((1 << tb.lg) - 1));
}

}  // namespace spa
