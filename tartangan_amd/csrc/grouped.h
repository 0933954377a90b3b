// Many small pieces of work ("items": one layer each) in ONE launch.  The table travels by value in the kernel argument
// block (nothing in memory to keep alive or copy); a workgroup finds its item by scanning <= MAX block offsets.  An entry
// point supplies an item struct, a row checker, a row -> item function and a kernel body; the rest is here.
#pragma once
#include "common.h"

template <class Item, int MAX>
struct TgGroupTable {
  using item_type = Item;
  static constexpr int max_items = MAX;
  int n;
  int block_end[MAX];                           // running end of the items' workgroup ranges
  Item item[MAX];
};

// The item of this workgroup (a reference: the item stays in the argument block) and the workgroup's offset inside it.
template <class Item, int MAX>
__device__ __forceinline__ const Item& tg_group_item(const TgGroupTable<Item, MAX>& t, int* local) {
  int i = 0;
  while (i + 1 < t.n && (int)blockIdx.x >= t.block_end[i]) ++i;        // uniform per workgroup
  *local = (int)blockIdx.x - (i > 0 ? t.block_end[i - 1] : 0);
  return t.item[i];
}

// Host side of every grouped entry point, over `n_rows` rows of `fields` host words:
//   check(row)        -> TG_OK / TG_EINVAL / TG_EUNSUPPORTED / TG_EWORKSPACE
//   fill(row, &item)  -> the item's workgroup count (int64; only called on rows that passed `check`)
//   launch(table, blocks)
// EVERY row is checked before the first launch, so a bad row leaves nothing written.  A launch takes at most MAX items and
// at most INT32_MAX workgroups (the grid index is 32 bits): the rest goes into the next one.  The tail of a table repeats
// item[0] with the final block_end.  The launch status is read after every launch; the first error ends the call.
template <class Table, class Check, class Fill, class Launch>
static int tg_group_run(const tg_host_i64* rows, int n_rows, int fields, Check check, Fill fill, Launch launch) {
  using Item = typename Table::item_type;
  constexpr int MAX = Table::max_items;
  static_assert(sizeof(Table) <= 4096, "the table travels in the kernel argument block");
  if (n_rows < 0) return TG_EINVAL;
  if (n_rows == 0) return TG_OK;
  TG_CHECK_PTR(rows);
  for (int r = 0; r < n_rows; ++r) {
    const tg_host_i64* row = rows + (size_t)r * fields;
    if (int rc = check(row)) return rc;
    Item probe;
    if (fill(row, &probe) > INT32_MAX) return TG_EUNSUPPORTED;
  }
  for (int base = 0; base < n_rows;) {
    Table t;
    int64_t blocks = 0;
    int n = 0;
    for (; n < MAX && base + n < n_rows; ++n) {
      Item it;
      const int64_t wgs = fill(rows + (size_t)(base + n) * fields, &it);
      if (n > 0 && blocks + wgs > INT32_MAX) break;
      t.item[n] = it;
      blocks += wgs;
      t.block_end[n] = (int)blocks;
    }
    t.n = n;
    for (int i = n; i < MAX; ++i) { t.item[i] = t.item[0]; t.block_end[i] = (int)blocks; }
    launch(t, (unsigned)blocks);
    if (int rc = tg_launch_status()) return rc;
    base += n;
  }
  return TG_OK;
}
