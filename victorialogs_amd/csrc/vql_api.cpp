// Product C-ABI for the MI355X-native block-scan engine.
//
// This is the drop-in boundary described in SURVEY.md §8b: the exports mirror
// what a cgo shim bound to VictoriaLogs' filter.applyToBlockSearch interface
// (lib/logstorage/filter.go:8-20, invoked from block_search.go:215 inside the
// worker loop storage_search.go:1040-1066) would call.  Host code stages
// decoded column blocks into HBM; hand-written HIP kernels (scan_kernels.hip)
// evaluate the filter program and return row bitmaps bit-identical to the
// reference's bitmap layout (bitmap.go:113-125).
//
// There is NO CPU fallback here: every scan entry point requires a working
// HIP device and fails loudly otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <chrono>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "core/filter.h"
#include "core/bloom.h"
#include "core/match.h"
#include "core/op_serialize.h"
#include "core/tokenizer.h"
#include "core/unicode_case.h"
#include "core/part_reader.h"
#include "core/values.h"
#include "hip/scan_types.h"

namespace vl {
extern "C" int vql_set_local_tz_nsecs(long long);
extern "C" hipError_t vql_launch_scan(const DevOp*, int, const DevLeafBlock*, int,
                                      const DevBlock*, const DevChunk*, uint32_t,
                                      unsigned long long*, hipStream_t);
extern "C" hipError_t vql_launch_gather_count(const DevGatherCol*, const DevBlock*,
                                              const DevChunk*, uint32_t,
                                              DevChunkCount*, hipStream_t);
extern "C" hipError_t vql_launch_gather_copy(const DevGatherCol*, const DevBlock*,
                                             const DevChunk*, uint32_t,
                                             const DevChunkBase*, uint8_t*,
                                             unsigned long long*,
                                             unsigned long long*, hipStream_t);
}

using namespace vl;

namespace {

thread_local std::string g_err;

#define HIP_CHECK(x)                                                         \
  do {                                                                       \
    hipError_t err__ = (x);                                                  \
    if (err__ != hipSuccess) {                                               \
      fail(std::string("HIP error: ") + hipGetErrorString(err__) + " at " + \
           #x);                                                              \
    }                                                                        \
  } while (0)

struct VqlPart {
  PartReader pr;
  std::vector<BlockHeader> bhs;
  explicit VqlPart(const std::string& dir) : pr(dir) {
    bhs = pr.read_all_block_headers();
  }
};

// Flattened program: postfix ops over leaf indices.
struct VqlFilter {
  FilterNode root;
  std::vector<const FilterNode*> leaves;
  std::vector<DevOp> ops;
  int max_depth = 0;

  explicit VqlFilter(FilterNode&& r) : root(std::move(r)) {
    int depth = flatten(root);
    max_depth = depth;
    if (int(ops.size()) > kMaxProgOps) fail("filter program too long");
    if (max_depth > kMaxStackDepth) fail("filter tree too deep (max 8)");
  }

  int flatten(const FilterNode& n) {
    switch (n.type) {
      case FilterNode::And:
      case FilterNode::Or: {
        if (n.children.empty()) fail("empty and/or");
        if (n.children.size() > 250) fail("too many and/or children");
        int d = 0;
        for (size_t i = 0; i < n.children.size(); i++) {
          // child i evaluates on top of i already-pushed results
          d = std::max(d, int(i) + flatten(n.children[i]));
        }
        DevOp op;
        op.kind = n.type == FilterNode::And ? kOpAnd : kOpOr;
        op.nargs = uint8_t(n.children.size());
        op.leaf = 0;
        ops.push_back(op);
        return d;
      }
      case FilterNode::Not: {
        int d = flatten(n.children[0]);
        DevOp op;
        op.kind = kOpNot;
        op.nargs = 1;
        op.leaf = 0;
        ops.push_back(op);
        return d;
      }
      default: {
        DevOp op;
        op.kind = kOpLeaf;
        op.nargs = 0;
        op.leaf = uint16_t(leaves.size());
        leaves.push_back(&n);
        ops.push_back(op);
        return 1;
      }
    }
  }
};




struct LeafInfo {
  const FilterNode* node;
  std::string cname;          // canonical column name
  bytes operand;              // phrase/value bytes or regex blob
  uint8_t phrase_flags = 0;
  // device pointer (filled at stage time)
  const uint8_t* d_operand = nullptr;
};

struct Stage {
  VqlPart* part;                      // first part (compat)
  std::shared_ptr<VqlFilter> filter;  // keep alive
  int device = 0;
  long lo = 0, hi = 0;                // single-part ranges (compat)
  // every staged block: (part, block index) — multi-part stages scan all of
  // them in ONE kernel launch (the reference worker model batches blocks
  // without caring which part they came from, storage_search.go:1035-1067)
  std::vector<std::pair<VqlPart*, long>> block_refs;

  // Slab arena: device memory grows with what is actually staged (the whole
  // part's uncompressed size is NOT a usable bound once only the filter's
  // columns are staged — a 1B-row part holds ~350 GB of columns of which the
  // or8 config stages ~265 GB into the 288 GB of HBM3E).  Slabs are never
  // reallocated, so staged pointers stay valid; every in-slab allocation
  // keeps >= kSlabTailPad bytes of owned slab memory after it (the string
  // tile copy rounds groups up to 1 KiB strides and may over-read).
  // 256 MiB: small enough that the per-stage tail waste stays negligible
  // even when a 1B-row config streams through 64 separate part-stages
  // (1 GiB slabs wasted ~32 GB there and OOM'd a 288 GiB device)
  static constexpr size_t kSlabBytes = size_t(256) << 20;
  static constexpr size_t kSlabTailPad = 4096;
  std::vector<std::pair<uint8_t*, size_t>> slabs;  // (ptr, capacity)
  uint8_t* cur_slab = nullptr;
  size_t cur_cap = 0, cur_used = 0;

  DevOp* d_ops = nullptr;
  DevLeafBlock* d_lbs = nullptr;
  DevBlock* d_blocks = nullptr;
  DevChunk* d_chunks = nullptr;
  unsigned long long* d_hits = nullptr;
  unsigned long long* d_block_hits = nullptr;
  uint64_t* d_bitmap = nullptr;
  size_t bitmap_words = 0;
  uint32_t nchunks = 0;

  std::vector<uint64_t> block_word_off;
  uint64_t staged_bytes = 0;   // bytes resident in HBM
  uint64_t algo_bytes = 0;     // algorithmic bytes one scan pass must read
  uint64_t rows = 0;
  uint64_t live_rows = 0;      // rows of blocks that actually reach the kernel

  // bitmap word ranges of statically-eliminated blocks (program value 0):
  // zeroed once on the first scan instead of dispatching their chunks
  std::vector<std::pair<uint64_t, uint64_t>> zero_word_ranges;
  bool bitmap_zeroed = false;

  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double last_kernel_ms = 0;

  // gather caches (blockResult materialization, §8f row 1)
  struct GatherCtx {
    DevGatherCol* d_gcols = nullptr;
    DevChunkBase* d_bases = nullptr;
    uint64_t nrows = 0, nbytes = 0;
    bool sized = false;
  };
  std::map<std::string, GatherCtx> gathers;
  std::vector<DevChunk> chunks_h;          // kept for gather passes
  std::vector<uint32_t> block_rows_h;      // rows per staged block

  ~Stage() {
    for (auto& kv : gathers) {
      if (kv.second.d_gcols) (void)hipFree(kv.second.d_gcols);
      if (kv.second.d_bases) (void)hipFree(kv.second.d_bases);
    }
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
    for (auto& s : slabs) (void)hipFree(s.first);
    if (d_ops) (void)hipFree(d_ops);
    if (d_lbs) (void)hipFree(d_lbs);
    if (d_blocks) (void)hipFree(d_blocks);
    if (d_chunks) (void)hipFree(d_chunks);
    if (d_hits) (void)hipFree(d_hits);
    if (d_block_hits) (void)hipFree(d_block_hits);
  }

  uint8_t* push(const void* src, size_t n, size_t align = 16) {
    uint8_t* dst = reserve(n, align);
    if (n) HIP_CHECK(hipMemcpy(dst, src, n, hipMemcpyHostToDevice));
    staged_bytes += n;
    return dst;
  }
  uint8_t* reserve(size_t n, size_t align = 16) {
    size_t used = (cur_used + align - 1) & ~(align - 1);
    if (cur_slab == nullptr || used + n + kSlabTailPad > cur_cap) {
      const size_t cap = std::max(kSlabBytes, n + kSlabTailPad + align);
      uint8_t* p = nullptr;
      HIP_CHECK(hipMalloc(&p, cap));
      slabs.emplace_back(p, cap);
      cur_slab = p;
      cur_cap = cap;
      cur_used = 0;
      used = 0;
    }
    uint8_t* dst = cur_slab + used;
    cur_used = used + n;
    return dst;
  }

  // bump-allocator watermark for statically-eliminated block rollback
  struct ArenaMark {
    size_t nslabs;
    uint8_t* cur_slab;
    size_t cur_cap, cur_used;
    uint64_t staged_bytes;
  };
  ArenaMark mark() const {
    return {slabs.size(), cur_slab, cur_cap, cur_used, staged_bytes};
  }
  void rollback(const ArenaMark& m) {
    while (slabs.size() > m.nslabs) {
      (void)hipFree(slabs.back().first);
      slabs.pop_back();
    }
    cur_slab = m.cur_slab;
    cur_cap = m.cur_cap;
    cur_used = m.cur_used;
    staged_bytes = m.staged_bytes;
  }
};

// Per-block staging caches
struct StagedStrCol {
  bool is_const = false;
  std::string const_value;
  const uint8_t* d_data = nullptr;
  const uint32_t* d_offsets = nullptr;
  uint64_t data_bytes = 0;
  uint64_t rows = 0;
  uint32_t sg = 1;  // small-row super-group size (DevLeafBlock.sg)
};

// Small-row super-group size for a string column: the largest sg in {8,4,2}
// for which the block's ACTUAL super-group byte spans (sg*64 rows counted
// from row 0, start rounded down to the tile copy's 16-byte alignment) fit
// one wave tile, allowing at most max(1, nsg/32) overflowing super-groups —
// those take the kernel's per-super-group global fallback, bit-identically.
// 1 = per-word tile loop.
static uint32_t pick_super_group(const std::vector<uint32_t>& offs,
                                 uint64_t rows) {
  if (rows == 0 || offs.size() < rows + 1) return 1;
  const uint64_t nwords = (rows + 63) / 64;
  for (uint32_t sg = 8; sg >= 2; sg /= 2) {
    const uint64_t nsg = (nwords + sg - 1) / sg;
    const uint64_t cap = std::max<uint64_t>(1, nsg / 32);
    uint64_t over = 0;
    for (uint64_t g = 0; g < nsg && over <= cap; g++) {
      const uint64_t ra = g * sg * 64;
      const uint64_t rb = std::min<uint64_t>(rows, ra + uint64_t(sg) * 64);
      const uint64_t span = uint64_t(offs[rb]) - (uint64_t(offs[ra]) & ~15ull);
      if (span > kWaveTileBytes) over++;
    }
    if (over <= cap) return sg;
  }
  return 1;
}

struct BlockStageCtx {
  Stage* st;
  const PartReader* pr;
  const BlockHeader* bh;
  PartReader::BlockColumns bc;
  std::map<std::string, StagedStrCol> cols;
  std::map<std::string, std::vector<uint64_t>> host_blooms;
  const int64_t* d_ts = nullptr;
  // the column the leaf being staged uploaded itself (if has_fresh; _msg is
  // stored under the empty name), and the arena as it was before: a
  // bloom-gate miss takes the upload back
  bool has_fresh = false;
  std::string fresh_col;
  Stage::ArenaMark fresh_mark{};

  const StagedStrCol& stage_column(const ColumnHeader& ch) {
    auto it = cols.find(ch.name);
    if (it != cols.end()) return it->second;
    StringsBlockDec dec;
    pr->read_values(ch, bh->rows_count, dec);
    StagedStrCol sc;
    sc.rows = bh->rows_count;
    if (dec.is_const) {
      sc.is_const = true;
      sc.const_value.assign((const char*)dec.data.data(), dec.data.size());
    } else {
      has_fresh = true;
      fresh_col = ch.name;
      fresh_mark = st->mark();
      sc.d_data = st->push(dec.data.data(), dec.data.size());
      // the tile copy rounds groups up to full 64-slot (1 KiB) strides and
      // may read up to ~1 KiB past the group end
      st->reserve(1024);
      sc.d_offsets = (const uint32_t*)st->push(dec.offsets.data(),
                                               dec.offsets.size() * 4, 4);
      sc.data_bytes = dec.data.size();
      sc.sg = pick_super_group(dec.offsets, sc.rows);
    }
    return cols.emplace(ch.name, std::move(sc)).first->second;
  }

  const std::vector<uint64_t>& bloom_host(const ColumnHeader& ch) {
    auto it = host_blooms.find(ch.name);
    if (it == host_blooms.end()) {
      std::vector<uint64_t> words;
      pr->read_bloom(ch, words);
      it = host_blooms.emplace(ch.name, std::move(words)).first;
    }
    return it->second;
  }

  const int64_t* stage_timestamps() {
    if (!d_ts) {
      std::vector<int64_t> ts;
      pr->read_timestamps(*bh, ts);
      d_ts = (const int64_t*)st->push(ts.data(), ts.size() * 8, 8);
    }
    return d_ts;
  }
};

bool h_bloom_all(BlockStageCtx& ctx, const ColumnHeader& ch,
                 const std::vector<uint64_t>& hashes);

// The leaf's bloom gate (bloomfilter.go:173-191), decided here on the host: a
// Stage binds one filter to one set of blocks, so the verdict never changes
// between scans.  Called at every gated leaf kind after the descriptor is
// filled.  A hit leaves the leaf as staged; a miss (the block cannot hold the
// leaf's tokens) makes it kModeNone for this block, which the static program
// evaluation then uses to drop whole blocks.  An empty hash list and a column
// without bloom words both pass, as containsAll does.  A column that only
// this leaf uploaded is taken back out of the arena on a miss.
void set_bloom_gate(DevLeafBlock& lb, BlockStageCtx& ctx, const ColumnHeader& ch,
                    const LeafInfo& li) {
  if (h_bloom_all(ctx, ch, li.node->token_hashes)) return;
  lb = DevLeafBlock{};
  lb.mode = kModeNone;
  if (ctx.has_fresh && ctx.fresh_col == ch.name) {
    ctx.st->rollback(ctx.fresh_mark);
    ctx.cols.erase(ch.name);
    ctx.has_fresh = false;
  }
}

// Shared helper: fixed-width binary equality with header min/max prune
// (filter_exact.go:296-354).  Returns true if staged as SCAN; false => NONE.
bool stage_eq_bin(DevLeafBlock& lb, BlockStageCtx& ctx, const ColumnHeader& ch,
                  const LeafInfo& li, Stage& st, const bytes& bin) {
  const StagedStrCol& sc = ctx.stage_column(ch);
  if (sc.is_const) {
    lb.mode = sc.const_value.size() == bin.size() &&
                      memcmp(sc.const_value.data(), bin.data(), bin.size()) == 0
                  ? kModeAll
                  : kModeNone;
    // NB: the reference would bloom-gate first; a bloom miss implies no match,
    // so host equality gives the identical verdict.
    return false;
  }
  lb.mode = kModeScan;
  lb.kind = kScanEqBin;
  lb.width = uint8_t(bin.size());
  lb.operand = (const uint8_t*)st.push(bin.data(), bin.size(), 8);
  lb.operand_len = uint32_t(bin.size());
  lb.data = sc.d_data;
  set_bloom_gate(lb, ctx, ch, li);
  return lb.mode == kModeScan;
}

// Binary equality without the leaf's own bloom gate (the set-family filters
// run their gate themselves).
void stage_eq_bin_nogate(DevLeafBlock& lb, BlockStageCtx& ctx,
                         const ColumnHeader& ch, Stage& st, const bytes& bin) {
  const StagedStrCol& sc = ctx.stage_column(ch);
  if (sc.is_const) {
    lb.mode = sc.const_value.size() == bin.size() &&
                      memcmp(sc.const_value.data(), bin.data(), bin.size()) == 0
                  ? kModeAll
                  : kModeNone;
    return;
  }
  lb.mode = kModeScan;
  lb.kind = kScanEqBin;
  lb.width = uint8_t(bin.size());
  lb.operand = (const uint8_t*)st.push(bin.data(), bin.size(), 8);
  lb.operand_len = uint32_t(bin.size());
  lb.data = sc.d_data;
}

bool in_sorted_bin_host(const std::vector<std::string>& sorted_set, strview v) {
  size_t lo = 0, hi = sorted_set.size();
  while (lo < hi) {
    size_t mid = (lo + hi) / 2;
    const std::string& m = sorted_set[mid];
    int c = memcmp(m.data(), v.p, std::min(m.size(), v.n));
    if (c == 0) c = m.size() < v.n ? -1 : (m.size() > v.n ? 1 : 0);
    if (c == 0) return true;
    if (c < 0) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return false;
}

// Returns the parsed+pruned binary value for exact matches on binary columns,
// or empty when the block is pruned (filter_exact.go:237-364).
bool exact_bin_value(const ColumnHeader& ch, strview value, bytes& bin) {
  switch (ch.type) {
    case ValueType::Uint8:
    case ValueType::Uint16:
    case ValueType::Uint32:
    case ValueType::Uint64: {
      uint64_t n;
      if (!try_parse_uint64(value, &n) || n < ch.min_value || n > ch.max_value) {
        return false;
      }
      if (ch.type == ValueType::Uint8) bin.push_back(uint8_t(n));
      else if (ch.type == ValueType::Uint16) put_u16be(bin, uint16_t(n));
      else if (ch.type == ValueType::Uint32) put_u32be(bin, uint32_t(n));
      else put_u64be(bin, n);
      return true;
    }
    case ValueType::Int64: {
      int64_t n;
      if (!try_parse_int64(value, &n) || n < int64_t(ch.min_value) ||
          n > int64_t(ch.max_value)) {
        return false;
      }
      put_i64be_zigzag(bin, n);
      return true;
    }
    case ValueType::Float64: {
      double f, mn, mx;
      uint64_t mnu = ch.min_value, mxu = ch.max_value;
      memcpy(&mn, &mnu, 8);
      memcpy(&mx, &mxu, 8);
      if (!try_parse_float64_exact(value, &f) || f < mn || f > mx) return false;
      uint64_t u;
      memcpy(&u, &f, 8);
      put_u64be(bin, u);
      return true;
    }
    case ValueType::IPv4: {
      uint32_t n;
      if (!try_parse_ipv4(value, &n) || uint64_t(n) < ch.min_value ||
          uint64_t(n) > ch.max_value) {
        return false;
      }
      put_u32be(bin, n);
      return true;
    }
    case ValueType::TimestampISO8601: {
      int64_t n;
      if (!try_parse_timestamp_iso8601(value, &n) || n < int64_t(ch.min_value) ||
          n > int64_t(ch.max_value)) {
        return false;
      }
      put_u64be(bin, uint64_t(n));
      return true;
    }
    default:
      fail("exact_bin_value: not a binary column");
  }
}

uint32_t dict_mask_of(const std::vector<std::string>& dict,
                      const std::function<bool(strview)>& pred) {
  uint32_t mask = 0;
  for (size_t i = 0; i < dict.size(); i++) {
    if (pred(strview(dict[i]))) mask |= uint32_t(1) << i;
  }
  return mask;
}

void stage_dict(DevLeafBlock& lb, BlockStageCtx& ctx, const ColumnHeader& ch,
                uint32_t mask) {
  if (mask == 0) {
    lb.mode = kModeNone;  // matchEncodedValuesDict fast path (filter_phrase.go:273-277)
    return;
  }
  const StagedStrCol& sc = ctx.stage_column(ch);
  if (sc.is_const) {
    // all rows share one 1-byte encoded value
    uint8_t idx = sc.const_value.empty() ? 0 : uint8_t(sc.const_value[0]);
    lb.mode = ((mask >> idx) & 1) ? kModeAll : kModeNone;
    return;
  }
  lb.mode = kModeScan;
  lb.kind = kScanDict;
  lb.dict_mask = mask;
  lb.data = sc.d_data;
}

// formats one encoded fixed-width value like the reference's to*String helpers
std::string format_encoded(ValueType t, strview v) {
  std::string s;
  const uint8_t* p = (const uint8_t*)v.p;
  switch (t) {
    case ValueType::Uint8: format_uint64(s, p[0]); break;
    case ValueType::Uint16: format_uint64(s, get_u16be(p)); break;
    case ValueType::Uint32: format_uint64(s, get_u32be(p)); break;
    case ValueType::Uint64: format_uint64(s, get_u64be(p)); break;
    case ValueType::Int64: format_int64(s, get_i64be_zigzag(p)); break;
    case ValueType::Float64: {
      uint64_t u = get_u64be(p);
      double d;
      memcpy(&d, &u, 8);
      format_float64(s, d);
      break;
    }
    case ValueType::IPv4: format_ipv4(s, get_u32be(p)); break;
    case ValueType::TimestampISO8601:
      format_timestamp_iso8601(s, int64_t(get_u64be(p)));
      break;
    default:
      fail("format_encoded: unexpected type");
  }
  return s;
}


// ---- helpers for the set/range filter family ----

// sorted string set blob: u32 n, u32 offs[n+1], bytes (kScanInStr layout)

bool h_match_any_phrase(strview v, const std::vector<std::string>& phrases) {
  for (const auto& ph : phrases) {
    if (match_phrase(v, strview(ph))) return true;
  }
  return false;
}

bool h_match_all_phrases(strview v, const std::vector<std::string>& phrases) {
  for (const auto& ph : phrases) {
    if (ph.empty()) continue;  // filter_contains_all.go:310-321
    if (!match_phrase(v, strview(ph))) return false;
  }
  return true;
}

bool h_match_string_range(strview s, const std::string& mn,
                          const std::string& mx) {
  // matchStringRange (filter_string_range.go:225-229)
  auto cmp = [](strview a, const std::string& b) {
    int c = memcmp(a.p, b.data(), std::min(a.n, b.size()));
    if (c != 0) return c;
    return a.n < b.size() ? -1 : (a.n > b.size() ? 1 : 0);
  };
  return cmp(s, mn) >= 0 && cmp(s, mx) < 0;
}

uint64_t h_rune_count(strview s) {
  uint64_t n = 0;
  for (size_t i = 0; i < s.n; i++) {
    if ((uint8_t(s.p[i]) & 0xC0) != 0x80) n++;
  }
  return n;
}

bool h_in_values(const std::vector<std::string>& values, strview v) {
  for (const auto& s2 : values) {
    if (strview(s2) == v) return true;
  }
  return false;
}

bool h_bloom_all(BlockStageCtx& ctx, const ColumnHeader& ch,
                 const std::vector<uint64_t>& hashes) {
  if (hashes.empty()) return true;
  const auto& words = ctx.bloom_host(ch);
  return bloom_contains_all(words.data(), words.size(), hashes.data(),
                            hashes.size());
}

// matchBloomFilterAnyTokenSet (filter_in.go:202-218); block-level — a bloom
// miss implies zero matching rows, so host gating is result-identical
bool h_bloom_any_token_set(const FilterNode& f, BlockStageCtx& ctx,
                           const ColumnHeader& ch) {
  if (!h_bloom_all(ctx, ch, f.common_hashes)) return false;
  if (f.set_hashes.size() > 1000 ||
      f.set_hashes.size() > 10 * ctx.bh->rows_count) {
    return true;
  }
  const auto& words = ctx.bloom_host(ch);
  for (const auto& hs : f.set_hashes) {
    if (bloom_contains_all(words.data(), words.size(), hs.data(), hs.size())) {
      return true;
    }
  }
  return false;
}

int bin_set_slot(ValueType t) {
  switch (t) {
    case ValueType::Uint8: return 0;
    case ValueType::Uint16: return 1;
    case ValueType::Uint32: return 2;
    case ValueType::Uint64: return 3;
    case ValueType::Int64: return 4;
    case ValueType::Float64: return 5;
    case ValueType::IPv4: return 6;
    case ValueType::TimestampISO8601: return 7;
    default: return -1;
  }
}

const char* value_type_name(ValueType t) {
  // filterValueType names (filter_value_type.go:44-67)
  switch (t) {
    case ValueType::String: return "string";
    case ValueType::Dict: return "dict";
    case ValueType::Uint8: return "uint8";
    case ValueType::Uint16: return "uint16";
    case ValueType::Uint32: return "uint32";
    case ValueType::Uint64: return "uint64";
    case ValueType::Int64: return "int64";
    case ValueType::Float64: return "float64";
    case ValueType::IPv4: return "ipv4";
    case ValueType::TimestampISO8601: return "iso8601";
    default: return "unknown";
  }
}

uint8_t fmt_of_type(ValueType t) {
  switch (t) {
    case ValueType::Uint8:
    case ValueType::Uint16:
    case ValueType::Uint32:
    case ValueType::Uint64: return kFmtU64;
    case ValueType::Int64: return kFmtI64;
    case ValueType::Float64: return kFmtF64;
    case ValueType::IPv4: return kFmtIp;
    case ValueType::TimestampISO8601: return kFmtIso;
    default: return 0;
  }
}

uint8_t width_of_type(ValueType t) {
  switch (t) {
    case ValueType::Uint8: return 1;
    case ValueType::Uint16: return 2;
    case ValueType::Uint32: return 4;
    case ValueType::IPv4: return 4;
    default: return 8;
  }
}

// stage one (leaf, block) descriptor; mirrors the oracle's apply_* dispatch.
void stage_leaf(const LeafInfo& li, BlockStageCtx& ctx, Stage& st, DevLeafBlock& lb) {
  const FilterNode& f = *li.node;
  const PartReader& pr = *ctx.pr;
  memset(&lb, 0, sizeof(lb));
  ctx.has_fresh = false;  // columns cached by earlier leaves stay

  auto const_val = [&]() -> std::string {
    std::string v;
    if (!pr.get_const_column(ctx.bc, li.cname, &v)) return "";
    return v;
  };

  switch (f.type) {
    case FilterNode::Noop:
      lb.mode = kModeAll;
      return;

    case FilterNode::Time: {
      // filter_time.go:114-137
      const TimestampsHeader& th = ctx.bh->timestamps_header;
      if (f.min_ts > f.max_ts || f.min_ts > th.max_timestamp ||
          f.max_ts < th.min_timestamp) {
        lb.mode = kModeNone;
        return;
      }
      if (f.min_ts <= th.min_timestamp && f.max_ts >= th.max_timestamp) {
        lb.mode = kModeAll;
        return;
      }
      lb.mode = kModeScan;
      lb.kind = kScanTsRange;
      lb.ts = ctx.stage_timestamps();
      lb.vmin = uint64_t(f.min_ts);
      lb.vmax = uint64_t(f.max_ts);
      return;
    }

    case FilterNode::Phrase: {
      strview phrase(f.phrase);
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = match_phrase(strview(cv), phrase) ? kModeAll : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = phrase.n > 0 ? kModeNone : kModeAll;  // filter_phrase.go:76-83
        return;
      }
      switch (ch.type) {
        case ValueType::String: {
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            lb.mode = match_phrase(strview(sc.const_value), phrase) ? kModeAll
                                                                    : kModeNone;
            return;
          }
          lb.mode = kModeScan;
          lb.kind = kScanPhraseStr;
          lb.flags = li.phrase_flags;
          lb.operand = li.d_operand;
          lb.operand_len = uint32_t(phrase.n);
          lb.data = sc.d_data;
          lb.offsets = sc.d_offsets;
          set_bloom_gate(lb, ctx, ch, li);
          return;
        }
        case ValueType::Dict: {
          uint32_t mask = dict_mask_of(
              ch.dict, [&](strview dv) { return match_phrase(dv, phrase); });
          stage_dict(lb, ctx, ch, mask);
          return;
        }
        case ValueType::Uint8:
        case ValueType::Uint16:
        case ValueType::Uint32:
        case ValueType::Uint64:
        case ValueType::Int64: {
          bytes bin;
          if (!exact_bin_value(ch, phrase, bin)) {
            lb.mode = kModeNone;
            return;
          }
          stage_eq_bin(lb, ctx, ch, li, st, bin);
          return;
        }
        case ValueType::Float64: {
          // matchFloat64ByPhrase (filter_phrase.go:159-186)
          double ff;
          bool ok = try_parse_float64_exact(phrase, &ff);
          bool special = f.phrase == "." || f.phrase == "+" || f.phrase == "-";
          if (!ok && !special) {
            lb.mode = kModeNone;
            return;
          }
          const char* dot =
              phrase.n ? (const char*)memchr(phrase.p, '.', phrase.n) : nullptr;
          long nd = dot ? dot - phrase.p : -1;
          if (nd > 0 && size_t(nd) < phrase.n - 1) {
            bytes bin;
            if (!exact_bin_value(ch, phrase, bin)) {
              lb.mode = kModeNone;
              return;
            }
            stage_eq_bin(lb, ctx, ch, li, st, bin);
            return;
          }
          // slow path: per-row Ryu formatting + matchPhrase on device
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            std::string fs;
            uint64_t u = get_u64be((const uint8_t*)sc.const_value.data());
            double d;
            memcpy(&d, &u, 8);
            format_float64(fs, d);
            lb.mode = match_phrase(strview(fs), phrase) ? kModeAll : kModeNone;
            return;
          }
          lb.mode = kModeScan;
          lb.kind = kScanPhraseF64;
          lb.width = 8;
          lb.flags = li.phrase_flags;
          lb.operand = li.d_operand;
          lb.operand_len = uint32_t(phrase.n);
          lb.data = sc.d_data;
          set_bloom_gate(lb, ctx, ch, li);
          return;
        }
        case ValueType::IPv4: {
          uint32_t ip;
          if (try_parse_ipv4(phrase, &ip)) {
            bytes bin;
            if (!exact_bin_value(ch, phrase, bin)) {
              lb.mode = kModeNone;
              return;
            }
            stage_eq_bin(lb, ctx, ch, li, st, bin);
            return;
          }
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            std::string s;
            format_ipv4(s, get_u32be((const uint8_t*)sc.const_value.data()));
            lb.mode = match_phrase(strview(s), phrase) ? kModeAll : kModeNone;
            return;
          }
          lb.mode = kModeScan;
          lb.kind = kScanPhraseIp;
          lb.flags = li.phrase_flags;
          lb.operand = li.d_operand;
          lb.operand_len = uint32_t(phrase.n);
          lb.data = sc.d_data;
          set_bloom_gate(lb, ctx, ch, li);
          return;
        }
        case ValueType::TimestampISO8601: {
          int64_t ts;
          if (try_parse_timestamp_iso8601(phrase, &ts)) {
            bytes bin;
            if (!exact_bin_value(ch, phrase, bin)) {
              lb.mode = kModeNone;
              return;
            }
            stage_eq_bin(lb, ctx, ch, li, st, bin);
            return;
          }
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            std::string s;
            format_timestamp_iso8601(
                s, int64_t(get_u64be((const uint8_t*)sc.const_value.data())));
            lb.mode = match_phrase(strview(s), phrase) ? kModeAll : kModeNone;
            return;
          }
          lb.mode = kModeScan;
          lb.kind = kScanPhraseIso;
          lb.flags = li.phrase_flags;
          lb.operand = li.d_operand;
          lb.operand_len = uint32_t(phrase.n);
          lb.data = sc.d_data;
          set_bloom_gate(lb, ctx, ch, li);
          return;
        }
        default:
          fail("unknown valueType while staging phrase filter");
      }
    }

    case FilterNode::Exact: {
      strview value(f.phrase);
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = strview(cv) == value ? kModeAll : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = value.n > 0 ? kModeNone : kModeAll;
        return;
      }
      switch (ch.type) {
        case ValueType::String: {
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            lb.mode = strview(sc.const_value) == value ? kModeAll : kModeNone;
            return;
          }
          lb.mode = kModeScan;
          lb.kind = kScanEqStr;
          lb.operand = li.d_operand;
          lb.operand_len = uint32_t(value.n);
          lb.data = sc.d_data;
          lb.offsets = sc.d_offsets;
          set_bloom_gate(lb, ctx, ch, li);
          return;
        }
        case ValueType::Dict: {
          uint32_t mask =
              dict_mask_of(ch.dict, [&](strview dv) { return dv == value; });
          stage_dict(lb, ctx, ch, mask);
          return;
        }
        default: {
          bytes bin;
          if (!exact_bin_value(ch, value, bin)) {
            lb.mode = kModeNone;
            return;
          }
          stage_eq_bin(lb, ctx, ch, li, st, bin);
          return;
        }
      }
    }

    case FilterNode::Regexp: {
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = regex_match(f.re, strview(cv)) ? kModeAll : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = regex_match(f.re, strview("", 0)) ? kModeAll : kModeNone;
        return;
      }
      if (ch.type == ValueType::Dict) {
        uint32_t mask =
            dict_mask_of(ch.dict, [&](strview dv) { return regex_match(f.re, dv); });
        stage_dict(lb, ctx, ch, mask);
        return;
      }
      const StagedStrCol& sc = ctx.stage_column(ch);
      if (sc.is_const) {
        // evaluate the single encoded value on the host
        std::string s;
        strview v(sc.const_value);
        switch (ch.type) {
          case ValueType::String: s = sc.const_value; break;
          case ValueType::Uint8: format_uint64(s, uint8_t(v.p[0])); break;
          case ValueType::Uint16: format_uint64(s, get_u16be((const uint8_t*)v.p)); break;
          case ValueType::Uint32: format_uint64(s, get_u32be((const uint8_t*)v.p)); break;
          case ValueType::Uint64: format_uint64(s, get_u64be((const uint8_t*)v.p)); break;
          case ValueType::Int64: format_int64(s, get_i64be_zigzag((const uint8_t*)v.p)); break;
          case ValueType::Float64: {
            uint64_t u = get_u64be((const uint8_t*)v.p);
            double d;
            memcpy(&d, &u, 8);
            format_float64(s, d);
            break;
          }
          case ValueType::IPv4: format_ipv4(s, get_u32be((const uint8_t*)v.p)); break;
          case ValueType::TimestampISO8601:
            format_timestamp_iso8601(s, int64_t(get_u64be((const uint8_t*)v.p)));
            break;
          default: fail("unexpected const column type");
        }
        lb.mode = regex_match(f.re, strview(s)) ? kModeAll : kModeNone;
        return;
      }
      lb.mode = kModeScan;
      lb.operand = li.d_operand;
      lb.operand_len = uint32_t(li.operand.size());
      lb.data = sc.d_data;
      switch (ch.type) {
        case ValueType::String:
          lb.kind = kScanRegexStr;
          lb.offsets = sc.d_offsets;
          break;
        case ValueType::Uint8: lb.kind = kScanRegexU; lb.width = 1; break;
        case ValueType::Uint16: lb.kind = kScanRegexU; lb.width = 2; break;
        case ValueType::Uint32: lb.kind = kScanRegexU; lb.width = 4; break;
        case ValueType::Uint64: lb.kind = kScanRegexU; lb.width = 8; break;
        case ValueType::Int64: lb.kind = kScanRegexI; lb.width = 8; break;
        case ValueType::Float64: lb.kind = kScanRegexF64; lb.width = 8; break;
        case ValueType::IPv4: lb.kind = kScanRegexIp; lb.width = 4; break;
        case ValueType::TimestampISO8601: lb.kind = kScanRegexIso; lb.width = 8; break;
        default: fail("unknown valueType while staging regexp filter");
      }
      set_bloom_gate(lb, ctx, ch, li);  // last: a miss drops `sc`
      return;
    }

    case FilterNode::Range: {
      double min_v = f.min_f, max_v = f.max_f;
      if (min_v > max_v) {
        lb.mode = kModeNone;
        return;
      }
      std::string cv = const_val();
      if (!cv.empty()) {
        double x = parse_math_number(strview(cv));
        lb.mode = (x >= min_v && x <= max_v) ? kModeAll : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = kModeNone;  // filter_range.go:199-204
        return;
      }
      if (ch.type == ValueType::Dict) {
        uint32_t mask = dict_mask_of(ch.dict, [&](strview dv) {
          double x = parse_math_number(dv);
          return x >= min_v && x <= max_v;
        });
        stage_dict(lb, ctx, ch, mask);
        return;
      }
      if (ch.type == ValueType::String) {
        // matchStringByRange (filter_range.go:261-265): parseMathNumber per
        // row on device; no bloom gate in the reference either
        const StagedStrCol& sc = ctx.stage_column(ch);
        if (sc.is_const) {
          double x = parse_math_number(strview(sc.const_value));
          lb.mode = (x >= min_v && x <= max_v) ? kModeAll : kModeNone;
          return;
        }
        lb.mode = kModeScan;
        lb.kind = kScanRangeStr;
        lb.data = sc.d_data;
        lb.offsets = sc.d_offsets;
        uint64_t vmin, vmax;
        memcpy(&vmin, &min_v, 8);
        memcpy(&vmax, &max_v, 8);
        lb.vmin = vmin;
        lb.vmax = vmax;
        return;
      }

      auto clamp_u64 = [](double x) -> uint64_t {
        if (x < 0) return 0;
        if (x > double(UINT64_MAX)) return UINT64_MAX;
        return uint64_t(x);
      };
      auto clamp_i64 = [](double x) -> int64_t {
        if (x < double(INT64_MIN)) return INT64_MIN;
        if (x >= double(INT64_MAX)) return INT64_MAX;
        return int64_t(x);
      };
      auto clamp_u32 = [](double x) -> uint32_t {
        if (x < 0) return 0;
        if (x > double(UINT32_MAX)) return UINT32_MAX;
        return uint32_t(x);
      };

      const StagedStrCol* scp = nullptr;
      auto need_scan = [&](ScanKind kind, uint8_t width, uint64_t vmin,
                           uint64_t vmax, uint8_t flags = 0) {
        scp = &ctx.stage_column(ch);
        if (scp->is_const) {
          // const encoded value: evaluate on host with the same decode
          strview v(scp->const_value);
          bool m = false;
          const uint8_t* p = (const uint8_t*)v.p;
          switch (kind) {
            case kScanRangeU: {
              uint64_t x = width == 1 ? p[0]
                           : width == 2 ? get_u16be(p)
                           : width == 4 ? get_u32be(p) : get_u64be(p);
              m = x >= vmin && x <= vmax;
              break;
            }
            case kScanRangeI: {
              int64_t x = (flags & 1) ? int64_t(get_u64be(p)) : get_i64be_zigzag(p);
              m = x >= int64_t(vmin) && x <= int64_t(vmax);
              break;
            }
            case kScanRangeF: {
              uint64_t u = get_u64be(p);
              double x, mnd, mxd;
              memcpy(&x, &u, 8);
              memcpy(&mnd, &vmin, 8);
              memcpy(&mxd, &vmax, 8);
              m = x >= mnd && x <= mxd;
              break;
            }
            default: break;
          }
          lb.mode = m ? kModeAll : kModeNone;
          return;
        }
        lb.mode = kModeScan;
        lb.kind = uint8_t(kind);
        lb.width = width;
        lb.flags = flags;
        lb.vmin = vmin;
        lb.vmax = vmax;
        lb.data = scp->d_data;
      };

      switch (ch.type) {
        case ValueType::Uint8:
        case ValueType::Uint16:
        case ValueType::Uint32:
        case ValueType::Uint64: {
          uint64_t mn = clamp_u64(std::ceil(min_v));
          uint64_t mx = clamp_u64(std::floor(max_v));
          if (max_v < 0 || mn > ch.max_value || mx < ch.min_value) {
            lb.mode = kModeNone;
            return;
          }
          uint8_t w = ch.type == ValueType::Uint8 ? 1
                      : ch.type == ValueType::Uint16 ? 2
                      : ch.type == ValueType::Uint32 ? 4 : 8;
          need_scan(kScanRangeU, w, mn, mx);
          return;
        }
        case ValueType::Int64: {
          int64_t mn = clamp_i64(std::ceil(min_v));
          int64_t mx = clamp_i64(std::floor(max_v));
          if (mn > int64_t(ch.max_value) || mx < int64_t(ch.min_value)) {
            lb.mode = kModeNone;
            return;
          }
          need_scan(kScanRangeI, 8, uint64_t(mn), uint64_t(mx));
          return;
        }
        case ValueType::Float64: {
          double cmn, cmx;
          uint64_t mnu = ch.min_value, mxu = ch.max_value;
          memcpy(&cmn, &mnu, 8);
          memcpy(&cmx, &mxu, 8);
          if (min_v > cmx || max_v < cmn) {
            lb.mode = kModeNone;
            return;
          }
          uint64_t vmin, vmax;
          memcpy(&vmin, &min_v, 8);
          memcpy(&vmax, &max_v, 8);
          need_scan(kScanRangeF, 8, vmin, vmax);
          return;
        }
        case ValueType::IPv4: {
          uint32_t mn = clamp_u32(std::ceil(min_v));
          uint32_t mx = clamp_u32(std::floor(max_v));
          if (max_v < 0 || uint64_t(mn) > ch.max_value ||
              uint64_t(mx) < ch.min_value) {
            lb.mode = kModeNone;
            return;
          }
          need_scan(kScanRangeU, 4, mn, mx);
          return;
        }
        case ValueType::TimestampISO8601: {
          int64_t mn = clamp_i64(std::ceil(min_v));
          int64_t mx = clamp_i64(std::floor(max_v));
          if (max_v < 0 || mn > int64_t(ch.max_value) ||
              mx < int64_t(ch.min_value)) {
            lb.mode = kModeNone;
            return;
          }
          need_scan(kScanRangeI, 8, uint64_t(mn), uint64_t(mx), /*flags=*/1);
          return;
        }
        default:
          fail("unknown valueType while staging range filter");
      }
    }


    case FilterNode::Prefix: {
      // filterPrefix.applyToBlockSearch (filter_prefix.go:58-316)
      strview prefix(f.phrase);
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = match_prefix(strview(cv), prefix) ? kModeAll : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = kModeNone;  // filter_prefix.go:73-78
        return;
      }
      auto scan_fmt = [&](uint8_t fmt, uint8_t width, bool bloom) {
        const StagedStrCol& sc = ctx.stage_column(ch);
        if (sc.is_const) {
          std::string str = format_encoded(ch.type, strview(sc.const_value));
          lb.mode = match_prefix(strview(str), prefix) ? kModeAll : kModeNone;
          return;
        }
        lb.mode = kModeScan;
        lb.kind = kScanPrefixFmt;
        lb.width = width;
        lb.flags = uint8_t((li.phrase_flags & 15) | (fmt << 4));
        lb.operand = li.d_operand;
        lb.operand_len = uint32_t(prefix.n);
        lb.data = sc.d_data;
        if (bloom) set_bloom_gate(lb, ctx, ch, li);
      };
      switch (ch.type) {
        case ValueType::String: {
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            lb.mode = match_prefix(strview(sc.const_value), prefix) ? kModeAll
                                                                    : kModeNone;
            return;
          }
          lb.mode = kModeScan;
          lb.kind = kScanPrefixStr;
          lb.flags = li.phrase_flags;
          lb.operand = li.d_operand;
          lb.operand_len = uint32_t(prefix.n);
          lb.data = sc.d_data;
          lb.offsets = sc.d_offsets;
          set_bloom_gate(lb, ctx, ch, li);
          return;
        }
        case ValueType::Dict: {
          uint32_t mask = dict_mask_of(
              ch.dict, [&](strview dv) { return match_prefix(dv, prefix); });
          stage_dict(lb, ctx, ch, mask);
          return;
        }
        case ValueType::Uint8:
        case ValueType::Uint16:
        case ValueType::Uint32:
        case ValueType::Uint64: {
          // filter_prefix.go:200-285 (no bloom gate)
          if (prefix.n == 0) {
            lb.mode = kModeAll;
            return;
          }
          uint64_t n;
          if (!try_parse_uint64(prefix, &n) || n > ch.max_value) {
            lb.mode = kModeNone;
            return;
          }
          uint8_t w = ch.type == ValueType::Uint8 ? 1
                      : ch.type == ValueType::Uint16 ? 2
                      : ch.type == ValueType::Uint32 ? 4 : 8;
          scan_fmt(kFmtU64, w, false);
          return;
        }
        case ValueType::Int64: {
          if (prefix.n == 0) {
            lb.mode = kModeAll;
            return;
          }
          if (f.phrase != "-") {
            int64_t n;
            if (!try_parse_int64(prefix, &n) || n < int64_t(ch.min_value) ||
                n > int64_t(ch.max_value)) {
              lb.mode = kModeNone;
              return;
            }
          }
          scan_fmt(kFmtI64, 8, false);
          return;
        }
        case ValueType::Float64: {
          // filter_prefix.go:148-176
          if (prefix.n == 0) {
            lb.mode = kModeAll;
            return;
          }
          double ff;
          bool ok = try_parse_float64_exact(prefix, &ff);
          bool special = f.phrase == "." || f.phrase == "+" || f.phrase == "-" ||
                         prefix.p[0] == 'e' || prefix.p[0] == 'E';
          if (!ok && !special) {
            lb.mode = kModeNone;
            return;
          }
          scan_fmt(kFmtF64, 8, true);
          return;
        }
        case ValueType::IPv4:
          if (prefix.n == 0) {
            lb.mode = kModeAll;
            return;
          }
          scan_fmt(kFmtIp, 4, true);
          return;
        case ValueType::TimestampISO8601:
          if (prefix.n == 0) {
            lb.mode = kModeAll;
            return;
          }
          scan_fmt(kFmtIso, 8, true);
          return;
        default:
          fail("unknown valueType while staging prefix filter");
      }
    }

    case FilterNode::ExactPrefix: {
      // filterExactPrefix.applyToBlockSearch (filter_exact_prefix.go:52-277)
      strview prefix(f.phrase);
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = match_exact_prefix(strview(cv), prefix) ? kModeAll : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = prefix.n > 0 ? kModeNone : kModeAll;
        return;
      }
      auto scan_fmt = [&](uint8_t fmt, uint8_t width, bool bloom) {
        const StagedStrCol& sc = ctx.stage_column(ch);
        if (sc.is_const) {
          std::string str = format_encoded(ch.type, strview(sc.const_value));
          lb.mode =
              match_exact_prefix(strview(str), prefix) ? kModeAll : kModeNone;
          return;
        }
        lb.mode = kModeScan;
        lb.kind = kScanExactPrefixFmt;
        lb.width = width;
        lb.flags = uint8_t(fmt << 4);
        lb.operand = li.d_operand;
        lb.operand_len = uint32_t(prefix.n);
        lb.data = sc.d_data;
        if (bloom) set_bloom_gate(lb, ctx, ch, li);
      };
      switch (ch.type) {
        case ValueType::String: {
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            lb.mode = match_exact_prefix(strview(sc.const_value), prefix)
                          ? kModeAll
                          : kModeNone;
            return;
          }
          lb.mode = kModeScan;
          lb.kind = kScanExactPrefixStr;
          lb.operand = li.d_operand;
          lb.operand_len = uint32_t(prefix.n);
          lb.data = sc.d_data;
          lb.offsets = sc.d_offsets;
          set_bloom_gate(lb, ctx, ch, li);
          return;
        }
        case ValueType::Dict: {
          uint32_t mask = dict_mask_of(ch.dict, [&](strview dv) {
            return match_exact_prefix(dv, prefix);
          });
          stage_dict(lb, ctx, ch, mask);
          return;
        }
        case ValueType::Uint8:
        case ValueType::Uint16:
        case ValueType::Uint32:
        case ValueType::Uint64: {
          // matchMinMaxExactPrefix (filter_exact_prefix.go:255-273)
          if (prefix.n == 0) {
            lb.mode = kModeAll;
            return;
          }
          if (!f.token_hashes.empty()) {
            lb.mode = kModeNone;
            return;
          }
          uint64_t n;
          if (!try_parse_uint64(prefix, &n) || n > ch.max_value) {
            lb.mode = kModeNone;
            return;
          }
          uint8_t w = ch.type == ValueType::Uint8 ? 1
                      : ch.type == ValueType::Uint16 ? 2
                      : ch.type == ValueType::Uint32 ? 4 : 8;
          scan_fmt(kFmtU64, w, false);
          return;
        }
        case ValueType::Int64: {
          if (prefix.n == 0) {
            lb.mode = kModeAll;
            return;
          }
          if (!f.token_hashes.empty()) {
            lb.mode = kModeNone;
            return;
          }
          if (f.phrase != "-") {
            int64_t n;
            if (!try_parse_int64(prefix, &n) || n > int64_t(ch.max_value) ||
                n < int64_t(ch.min_value)) {
              lb.mode = kModeNone;
              return;
            }
          }
          scan_fmt(kFmtI64, 8, false);
          return;
        }
        case ValueType::Float64: {
          // filter_exact_prefix.go:136-153
          if (prefix.n == 0) {
            lb.mode = kModeAll;
            return;
          }
          if (f.token_hashes.size() > 2 * kBloomHashesCount) {
            lb.mode = kModeNone;
            return;
          }
          scan_fmt(kFmtF64, 8, true);
          return;
        }
        case ValueType::IPv4: {
          // filter_exact_prefix.go:119-134
          if (prefix.n == 0) {
            lb.mode = kModeAll;
            return;
          }
          if (f.phrase < "0" || f.phrase > "9" ||
              f.token_hashes.size() > 3 * kBloomHashesCount) {
            lb.mode = kModeNone;
            return;
          }
          scan_fmt(kFmtIp, 4, true);
          return;
        }
        case ValueType::TimestampISO8601: {
          // filter_exact_prefix.go:102-117
          if (prefix.n == 0) {
            lb.mode = kModeAll;
            return;
          }
          if (f.phrase < "0" || f.phrase > "9") {
            lb.mode = kModeNone;
            return;
          }
          scan_fmt(kFmtIso, 8, true);
          return;
        }
        default:
          fail("unknown valueType while staging exact_prefix filter");
      }
    }

    case FilterNode::Sequence: {
      // filterSequence.applyToBlockSearch (filter_sequence.go:84-258)
      const auto& phrases = f.phrases;
      if (phrases.empty()) {
        lb.mode = kModeAll;
        return;
      }
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = match_sequence(strview(cv), phrases) ? kModeAll : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode =
            match_sequence(strview("", 0), phrases) ? kModeAll : kModeNone;
        return;
      }
      switch (ch.type) {
        case ValueType::String: {
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            lb.mode = match_sequence(strview(sc.const_value), phrases)
                          ? kModeAll
                          : kModeNone;
            return;
          }
          lb.mode = kModeScan;
          lb.kind = kScanSeqStr;
          lb.operand = li.d_operand;
          lb.operand_len = uint32_t(li.operand.size());
          lb.data = sc.d_data;
          lb.offsets = sc.d_offsets;
          set_bloom_gate(lb, ctx, ch, li);
          return;
        }
        case ValueType::Dict: {
          uint32_t mask = dict_mask_of(
              ch.dict, [&](strview dv) { return match_sequence(dv, phrases); });
          stage_dict(lb, ctx, ch, mask);
          return;
        }
        case ValueType::Uint8:
        case ValueType::Uint16:
        case ValueType::Uint32:
        case ValueType::Uint64:
        case ValueType::Int64: {
          // filter_sequence.go:219-258: multi-phrase cannot match one number
          if (phrases.size() > 1) {
            lb.mode = kModeNone;
            return;
          }
          bytes bin;
          if (!exact_bin_value(ch, strview(phrases[0]), bin)) {
            lb.mode = kModeNone;
            return;
          }
          stage_eq_bin(lb, ctx, ch, li, st, bin);
          return;
        }
        case ValueType::Float64: {
          // matchFloat64BySequence (filter_sequence.go:179-196)
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            std::string str = format_encoded(ch.type, strview(sc.const_value));
            lb.mode = match_sequence(strview(str), phrases) ? kModeAll
                                                            : kModeNone;
            return;
          }
          lb.mode = kModeScan;
          lb.kind = kScanSeqFmt;
          lb.width = 8;
          lb.flags = uint8_t(kFmtF64 << 4);
          lb.operand = li.d_operand;
          lb.operand_len = uint32_t(li.operand.size());
          lb.data = sc.d_data;
          set_bloom_gate(lb, ctx, ch, li);
          return;
        }
        case ValueType::IPv4:
        case ValueType::TimestampISO8601: {
          if (phrases.size() == 1) {
            // delegate to the phrase matcher (filter_sequence.go:139-177)
            FilterNode tmp;
            tmp.type = FilterNode::Phrase;
            tmp.field = f.field;
            tmp.phrase = phrases[0];
            tmp.token_hashes = f.token_hashes;
            LeafInfo tmp_li;
            tmp_li.node = &tmp;
            tmp_li.cname = li.cname;
            tmp_li.operand.assign(phrases[0].begin(), phrases[0].end());
            tmp_li.phrase_flags = phrase_flags_of(phrases[0]);
            tmp_li.d_operand =
                (const uint8_t*)st.push(tmp_li.operand.data(),
                                        tmp_li.operand.size(), 8);
            stage_leaf(tmp_li, ctx, st, lb);
            return;
          }
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            std::string str = format_encoded(ch.type, strview(sc.const_value));
            lb.mode = match_sequence(strview(str), phrases) ? kModeAll
                                                            : kModeNone;
            return;
          }
          lb.mode = kModeScan;
          lb.kind = kScanSeqFmt;
          lb.width = ch.type == ValueType::IPv4 ? 4 : 8;
          lb.flags = uint8_t((ch.type == ValueType::IPv4 ? kFmtIp : kFmtIso) << 4);
          lb.operand = li.d_operand;
          lb.operand_len = uint32_t(li.operand.size());
          lb.data = sc.d_data;
          set_bloom_gate(lb, ctx, ch, li);
          return;
        }
        default:
          fail("unknown valueType while staging sequence filter");
      }
    }


    case FilterNode::In: {
      // filterIn (filter_in.go:120-234)
      if (f.values.empty()) {
        lb.mode = kModeNone;
        return;
      }
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = h_in_values(f.values, strview(cv)) ? kModeAll : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = h_in_values(f.values, strview("", 0)) ? kModeAll : kModeNone;
        return;
      }
      if (ch.type == ValueType::Dict) {
        uint32_t mask = dict_mask_of(
            ch.dict, [&](strview dv) { return h_in_values(f.values, dv); });
        stage_dict(lb, ctx, ch, mask);
        return;
      }
      if (ch.type == ValueType::String) {
        if (!h_bloom_any_token_set(f, ctx, ch)) {
          lb.mode = kModeNone;
          return;
        }
        const StagedStrCol& sc = ctx.stage_column(ch);
        if (sc.is_const) {
          lb.mode = h_in_values(f.values, strview(sc.const_value)) ? kModeAll
                                                                   : kModeNone;
          return;
        }
        lb.mode = kModeScan;
        lb.kind = kScanInStr;
        lb.operand = li.d_operand;  // sorted deduped string-set blob
        lb.operand_len = uint32_t(li.operand.size());
        lb.data = sc.d_data;
        lb.offsets = sc.d_offsets;
        return;
      }
      const auto& set = f.bin_sets[size_t(bin_set_slot(ch.type))];
      if (set.empty()) {
        lb.mode = kModeNone;
        return;
      }
      if (!h_bloom_any_token_set(f, ctx, ch)) {
        lb.mode = kModeNone;
        return;
      }
      const StagedStrCol& sc = ctx.stage_column(ch);
      uint8_t w = width_of_type(ch.type);
      if (sc.is_const) {
        lb.mode = in_sorted_bin_host(set, strview(sc.const_value)) ? kModeAll
                                                                   : kModeNone;
        return;
      }
      bytes packed;
      for (const auto& v : set) packed.insert(packed.end(), v.begin(), v.end());
      lb.mode = kModeScan;
      lb.kind = kScanInBin;
      lb.width = w;
      lb.operand = (const uint8_t*)st.push(packed.data(), packed.size(), 8);
      lb.operand_len = uint32_t(packed.size());
      lb.data = sc.d_data;
      return;
    }

    case FilterNode::ContainsAny: {
      // filterContainsAny (filter_contains_any.go:105-296)
      if (f.values.empty()) {
        lb.mode = kModeNone;
        return;
      }
      for (const auto& v : f.values) {
        if (v.empty()) {
          lb.mode = kModeAll;  // empty value matches everything (:110-113)
          return;
        }
      }
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = h_match_any_phrase(strview(cv), f.values) ? kModeAll
                                                            : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = h_match_any_phrase(strview("", 0), f.values) ? kModeAll
                                                               : kModeNone;
        return;
      }
      if (ch.type == ValueType::Dict) {
        uint32_t mask = dict_mask_of(ch.dict, [&](strview dv) {
          return h_match_any_phrase(dv, f.values);
        });
        stage_dict(lb, ctx, ch, mask);
        return;
      }
      if (ch.type == ValueType::Uint8 || ch.type == ValueType::Uint16 ||
          ch.type == ValueType::Uint32 || ch.type == ValueType::Uint64) {
        // uint columns match whole-value only (filter_contains_any.go:141-152)
        const auto& set = f.bin_sets[size_t(bin_set_slot(ch.type))];
        if (set.empty() || !h_bloom_any_token_set(f, ctx, ch)) {
          lb.mode = kModeNone;
          return;
        }
        const StagedStrCol& sc = ctx.stage_column(ch);
        uint8_t w = width_of_type(ch.type);
        if (sc.is_const) {
          lb.mode = in_sorted_bin_host(set, strview(sc.const_value)) ? kModeAll
                                                                     : kModeNone;
          return;
        }
        bytes packed;
        for (const auto& v : set) packed.insert(packed.end(), v.begin(), v.end());
        lb.mode = kModeScan;
        lb.kind = kScanInBin;
        lb.width = w;
        lb.operand = (const uint8_t*)st.push(packed.data(), packed.size(), 8);
        lb.operand_len = uint32_t(packed.size());
        lb.data = sc.d_data;
        return;
      }
      // common-token gate + per-value token-set survivor filter
      // (matchValuesAnyPhrase, filter_contains_any.go:179-198); survivor
      // filtering is result-identical: a bloom miss for value i means no row
      // contains all of i's tokens, so phrase i matches no row
      if (!h_bloom_all(ctx, ch, f.common_hashes)) {
        lb.mode = kModeNone;
        return;
      }
      std::vector<std::string> survivors;
      {
        const auto& words = ctx.bloom_host(ch);
        for (size_t i = 0; i < f.values.size(); i++) {
          if (bloom_contains_all(words.data(), words.size(),
                                 f.set_hashes[i].data(),
                                 f.set_hashes[i].size())) {
            survivors.push_back(f.values[i]);
          }
        }
      }
      if (survivors.empty()) {
        lb.mode = kModeNone;
        return;
      }
      const StagedStrCol& sc = ctx.stage_column(ch);
      if (sc.is_const) {
        std::string str = ch.type == ValueType::String
                              ? sc.const_value
                              : format_encoded(ch.type, strview(sc.const_value));
        lb.mode = h_match_any_phrase(strview(str), survivors) ? kModeAll
                                                              : kModeNone;
        return;
      }
      bytes blob = serialize_phrases(survivors);
      lb.mode = kModeScan;
      lb.operand = (const uint8_t*)st.push(blob.data(), blob.size(), 8);
      lb.operand_len = uint32_t(blob.size());
      lb.data = sc.d_data;
      if (ch.type == ValueType::String) {
        lb.kind = kScanAnyPhraseStr;
        lb.offsets = sc.d_offsets;
      } else {
        lb.kind = kScanAnyPhraseFmt;
        lb.width = width_of_type(ch.type);
        lb.flags = uint8_t(fmt_of_type(ch.type) << 4);
      }
      return;
    }

    case FilterNode::ContainsAll: {
      // filterContainsAll (filter_contains_all.go:123-321)
      bool only_empty = f.values.size() == 1 && f.values[0].empty();
      if (f.values.empty() || only_empty) {
        lb.mode = kModeAll;
        return;
      }
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = h_match_all_phrases(strview(cv), f.values) ? kModeAll
                                                             : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = h_match_all_phrases(strview("", 0), f.values) ? kModeAll
                                                                : kModeNone;
        return;
      }
      if (ch.type == ValueType::Dict) {
        uint32_t mask = dict_mask_of(ch.dict, [&](strview dv) {
          return h_match_all_phrases(dv, f.values);
        });
        stage_dict(lb, ctx, ch, mask);
        return;
      }
      if (ch.type == ValueType::Uint8 || ch.type == ValueType::Uint16 ||
          ch.type == ValueType::Uint32 || ch.type == ValueType::Uint64) {
        // matchAllValues (filter_contains_all.go:183-204)
        std::vector<std::string> distinct;
        for (const auto& v : f.values) {
          if (!v.empty() &&
              std::find(distinct.begin(), distinct.end(), v) == distinct.end()) {
            distinct.push_back(v);
          }
        }
        if (distinct.empty()) {
          lb.mode = kModeAll;
          return;
        }
        const auto& set = f.bin_sets[size_t(bin_set_slot(ch.type))];
        if (distinct.size() != 1 || set.size() != 1 ||
            !h_bloom_all(ctx, ch, f.all_hashes)) {
          lb.mode = kModeNone;
          return;
        }
        bytes bin(set[0].begin(), set[0].end());
        stage_eq_bin_nogate(lb, ctx, ch, st, bin);
        return;
      }
      if (!h_bloom_all(ctx, ch, f.all_hashes)) {
        lb.mode = kModeNone;
        return;
      }
      const StagedStrCol& sc = ctx.stage_column(ch);
      if (sc.is_const) {
        std::string str = ch.type == ValueType::String
                              ? sc.const_value
                              : format_encoded(ch.type, strview(sc.const_value));
        lb.mode = h_match_all_phrases(strview(str), f.values) ? kModeAll
                                                              : kModeNone;
        return;
      }
      lb.mode = kModeScan;
      lb.operand = li.d_operand;  // serialized phrase list
      lb.operand_len = uint32_t(li.operand.size());
      lb.data = sc.d_data;
      if (ch.type == ValueType::String) {
        lb.kind = kScanAllPhrasesStr;
        lb.offsets = sc.d_offsets;
      } else {
        lb.kind = kScanAllPhrasesFmt;
        lb.width = width_of_type(ch.type);
        lb.flags = uint8_t(fmt_of_type(ch.type) << 4);
      }
      return;
    }

    case FilterNode::StringRange: {
      // filterStringRange (filter_string_range.go:47-230)
      if (f.min_s > f.max_s) {
        lb.mode = kModeNone;
        return;
      }
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = h_match_string_range(strview(cv), f.min_s, f.max_s)
                      ? kModeAll
                      : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = h_match_string_range(strview("", 0), f.min_s, f.max_s)
                      ? kModeAll
                      : kModeNone;
        return;
      }
      // per-type prunes (filter_string_range.go:100-225)
      switch (ch.type) {
        case ValueType::String:
        case ValueType::Dict:
          break;
        case ValueType::Int64:
          if ((f.min_s != "-" && f.min_s > "9") ||
              (f.max_s != "-" && f.max_s < "0")) {
            lb.mode = kModeNone;
            return;
          }
          break;
        case ValueType::Float64:
          if (f.min_s > "9" || f.max_s < "+") {
            lb.mode = kModeNone;
            return;
          }
          break;
        default:
          if (f.min_s > "9" || f.max_s < "0") {
            lb.mode = kModeNone;
            return;
          }
          break;
      }
      if (ch.type == ValueType::Dict) {
        uint32_t mask = dict_mask_of(ch.dict, [&](strview dv) {
          return h_match_string_range(dv, f.min_s, f.max_s);
        });
        stage_dict(lb, ctx, ch, mask);
        return;
      }
      const StagedStrCol& sc = ctx.stage_column(ch);
      if (sc.is_const) {
        std::string str = ch.type == ValueType::String
                              ? sc.const_value
                              : format_encoded(ch.type, strview(sc.const_value));
        lb.mode = h_match_string_range(strview(str), f.min_s, f.max_s)
                      ? kModeAll
                      : kModeNone;
        return;
      }
      lb.mode = kModeScan;
      lb.operand = li.d_operand;  // u32 minlen, u32 maxlen, min, max
      lb.operand_len = uint32_t(li.operand.size());
      lb.data = sc.d_data;
      if (ch.type == ValueType::String) {
        lb.kind = kScanStrRange;
        lb.offsets = sc.d_offsets;
      } else {
        lb.kind = kScanStrRangeFmt;
        lb.width = width_of_type(ch.type);
        lb.flags = uint8_t(fmt_of_type(ch.type) << 4);
      }
      return;
    }

    case FilterNode::IPv4Range: {
      // filterIPv4Range (filter_ipv4_range.go:99-190)
      uint32_t mn = uint32_t(f.min_u), mx = uint32_t(f.max_u);
      if (mn > mx) {
        lb.mode = kModeNone;
        return;
      }
      auto match_str = [&](strview v) {
        uint32_t ip;
        if (!try_parse_ipv4(v, &ip)) return false;
        return ip >= mn && ip <= mx;
      };
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = match_str(strview(cv)) ? kModeAll : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = kModeNone;
        return;
      }
      switch (ch.type) {
        case ValueType::String: {
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            lb.mode = match_str(strview(sc.const_value)) ? kModeAll : kModeNone;
            return;
          }
          lb.mode = kModeScan;
          lb.kind = kScanIPv4RangeStr;
          lb.vmin = mn;
          lb.vmax = mx;
          lb.data = sc.d_data;
          lb.offsets = sc.d_offsets;
          return;
        }
        case ValueType::Dict: {
          uint32_t mask = dict_mask_of(ch.dict, match_str);
          stage_dict(lb, ctx, ch, mask);
          return;
        }
        case ValueType::IPv4: {
          // matchIPv4ByRange (filter_ipv4_range.go:166-181)
          if (ch.min_value > mx || ch.max_value < mn) {
            lb.mode = kModeNone;
            return;
          }
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            uint32_t ip = get_u32be((const uint8_t*)sc.const_value.data());
            lb.mode = (ip >= mn && ip <= mx) ? kModeAll : kModeNone;
            return;
          }
          lb.mode = kModeScan;
          lb.kind = kScanIPv4RangeBin;
          lb.width = 4;
          lb.vmin = mn;
          lb.vmax = mx;
          lb.data = sc.d_data;
          return;
        }
        default:
          lb.mode = kModeNone;
          return;
      }
    }

    case FilterNode::LenRange: {
      // filterLenRange (filter_len_range.go:126-348)
      uint64_t mn = f.min_u, mx = f.max_u;
      if (mn > mx) {
        lb.mode = kModeNone;
        return;
      }
      auto match_len = [&](strview v) {
        uint64_t n = h_rune_count(v);
        return n >= mn && n <= mx;
      };
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = match_len(strview(cv)) ? kModeAll : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = match_len(strview("", 0)) ? kModeAll : kModeNone;
        return;
      }
      // per-type prunes (filter_len_range.go:180-331)
      auto minmax_len_ok = [&]() {
        std::string s2;
        format_uint64(s2, ch.min_value);
        if (mx < s2.size()) return false;
        s2.clear();
        format_uint64(s2, ch.max_value);
        return mn <= s2.size();
      };
      switch (ch.type) {
        case ValueType::String:
          break;
        case ValueType::Dict: {
          uint32_t mask = dict_mask_of(ch.dict, match_len);
          stage_dict(lb, ctx, ch, mask);
          return;
        }
        case ValueType::Uint8:
          if (mn > 3 || mx == 0 || !minmax_len_ok()) {
            lb.mode = kModeNone;
            return;
          }
          break;
        case ValueType::Uint16:
          if (mn > 5 || mx == 0 || !minmax_len_ok()) {
            lb.mode = kModeNone;
            return;
          }
          break;
        case ValueType::Uint32:
          if (mn > 10 || mx == 0 || !minmax_len_ok()) {
            lb.mode = kModeNone;
            return;
          }
          break;
        case ValueType::Uint64:
          if (mn > 20 || mx == 0 || !minmax_len_ok()) {
            lb.mode = kModeNone;
            return;
          }
          break;
        case ValueType::Int64:
          if (mn > 20 || mx == 0) {
            lb.mode = kModeNone;
            return;
          }
          break;
        case ValueType::Float64:
          if (mn > 24 || mx == 0) {
            lb.mode = kModeNone;
            return;
          }
          break;
        case ValueType::IPv4:
          if (mn > 15 || mx < 7) {
            lb.mode = kModeNone;
            return;
          }
          break;
        case ValueType::TimestampISO8601:
          // formatted length is always 24 (filter_len_range.go:180-185)
          lb.mode = (mn <= 24 && mx >= 24) ? kModeAll : kModeNone;
          return;
        default:
          fail("unknown valueType while staging len_range filter");
      }
      const StagedStrCol& sc = ctx.stage_column(ch);
      if (sc.is_const) {
        std::string str = ch.type == ValueType::String
                              ? sc.const_value
                              : format_encoded(ch.type, strview(sc.const_value));
        lb.mode = match_len(strview(str)) ? kModeAll : kModeNone;
        return;
      }
      lb.mode = kModeScan;
      lb.vmin = mn;
      lb.vmax = mx;
      lb.data = sc.d_data;
      if (ch.type == ValueType::String) {
        lb.kind = kScanLenRangeStr;
        lb.offsets = sc.d_offsets;
      } else {
        lb.kind = kScanLenRangeFmt;
        lb.width = width_of_type(ch.type);
        lb.flags = uint8_t(fmt_of_type(ch.type) << 4);
      }
      return;
    }

    case FilterNode::DayRange:
    case FilterNode::WeekRange: {
      // filterDayRange / filterWeekRange (filter_day_range.go:126-139,
      // filter_week_range.go:128-141)
      int64_t start = int64_t(f.min_u), end = int64_t(f.max_u);
      if (start > end) {
        lb.mode = kModeNone;
        return;
      }
      const bool is_day = f.type == FilterNode::DayRange;
      const int64_t full_end = is_day ? 24LL * 3600 * 1000000000 - 1 : 6;
      if (start == 0 && end == full_end) {
        lb.mode = kModeAll;
        return;
      }
      lb.mode = kModeScan;
      lb.kind = is_day ? kScanDayRange : kScanWeekRange;
      lb.ts = ctx.stage_timestamps();
      lb.vmin = uint64_t(start);
      lb.vmax = uint64_t(end);
      lb.operand = li.d_operand;  // 8-byte tz offset
      lb.operand_len = 8;
      return;
    }

    case FilterNode::ValueTypeFilter: {
      // filterValueType (filter_value_type.go:44-67)
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = f.min_s == "const" ? kModeAll : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        lb.mode = kModeNone;
        return;
      }
      lb.mode = f.min_s == value_type_name(ch.type) ? kModeAll : kModeNone;
      return;
    }

    case FilterNode::StreamIdFilter: {
      // filterStreamID block gate (filter_stream_id.go:127-143)
      const StreamID& sid = ctx.bh->stream_id;
      uint64_t tp = uint64_t(sid.account_id) << 32 | sid.project_id;
      for (const auto& id : f.stream_ids) {
        if (id[0] == tp && id[1] == sid.id_hi && id[2] == sid.id_lo) {
          lb.mode = kModeAll;
          return;
        }
      }
      lb.mode = kModeNone;
      return;
    }


    case FilterNode::AnyCasePhrase:
    case FilterNode::AnyCasePrefix: {
      // filterAnyCasePhrase / filterAnyCasePrefix
      // (filter_any_case_phrase.go:85-138, filter_any_case_prefix.go:90-140)
      const bool is_ph = f.type == FilterNode::AnyCasePhrase;
      strview lower(f.min_s);
      auto host_match = [&](strview v) {
        return is_ph ? match_any_case_phrase(v, lower)
                     : match_any_case_prefix(v, lower);
      };
      std::string cv = const_val();
      if (!cv.empty()) {
        lb.mode = host_match(strview(cv)) ? kModeAll : kModeNone;
        return;
      }
      ColumnHeader ch;
      if (!pr.get_column_header(ctx.bc, li.cname, &ch)) {
        // phrase: empty phrase matches missing columns; prefix: never
        lb.mode = is_ph && lower.n == 0 ? kModeAll : kModeNone;
        return;
      }
      switch (ch.type) {
        case ValueType::String: {
          const StagedStrCol& sc = ctx.stage_column(ch);
          if (sc.is_const) {
            lb.mode = host_match(strview(sc.const_value)) ? kModeAll : kModeNone;
            return;
          }
          // rows with non-ASCII bytes need the full Unicode lowercase
          // mapping (AppendLowercase slow path) — resolve them on the host
          // at stage time; the kernel handles the ASCII rows
          StringsBlockDec dec;
          pr.read_values(ch, ctx.bh->rows_count, dec);
          const uint32_t rows = uint32_t(ctx.bh->rows_count);
          const size_t nw = (rows + 63) / 64;
          std::vector<uint64_t> mask(nw, 0), val(nw, 0);
          bool any = false;
          for (uint32_t r = 0; r < rows; r++) {
            const char* vp = (const char*)dec.data.data() + dec.offsets[r];
            const size_t vn = dec.offsets[r + 1] - dec.offsets[r];
            bool ascii = true;
            for (size_t k = 0; k < vn; k++) {
              if (uint8_t(vp[k]) >= 0x80) {
                ascii = false;
                break;
              }
            }
            if (ascii) continue;
            any = true;
            mask[r >> 6] |= uint64_t(1) << (r & 63);
            if (host_match(strview(vp, vn))) {
              val[r >> 6] |= uint64_t(1) << (r & 63);
            }
          }
          lb.mode = kModeScan;
          lb.kind = is_ph ? kScanAnyCasePhraseStr : kScanAnyCasePrefixStr;
          lb.flags = li.phrase_flags;  // flags of the lowercase phrase
          lb.operand = li.d_operand;
          lb.operand_len = uint32_t(f.min_s.size());
          lb.data = sc.d_data;
          lb.offsets = sc.d_offsets;
          if (any) {
            // override bitmaps ride in the side-data fields (scan_types.h
            // DevLeafBlock comment)
            lb.hashes = (const uint64_t*)st.push(mask.data(), nw * 8, 8);
            lb.bloom = (const uint64_t*)st.push(val.data(), nw * 8, 8);
          }
          return;
        }
        case ValueType::Dict: {
          uint32_t m = dict_mask_of(ch.dict, host_match);
          stage_dict(lb, ctx, ch, m);
          return;
        }
        default: {
          // numeric/ip/iso types: the stored values never contain letters in
          // mixed case, so the reference delegates to the exact/prefix
          // matchers with the lowercase (iso: uppercase) phrase
          const bool iso = ch.type == ValueType::TimestampISO8601;
          FilterNode tmp;
          tmp.type = is_ph ? FilterNode::Phrase : FilterNode::Prefix;
          tmp.field = f.field;
          tmp.phrase = iso ? f.max_s : f.min_s;
          tmp.token_hashes = iso ? f.all_hashes : f.token_hashes;
          LeafInfo tmp_li;
          tmp_li.node = &tmp;
          tmp_li.cname = li.cname;
          tmp_li.operand.assign(tmp.phrase.begin(), tmp.phrase.end());
          tmp_li.phrase_flags = phrase_flags_of(tmp.phrase);
          if (!tmp_li.operand.empty()) {
            tmp_li.d_operand = (const uint8_t*)st.push(tmp_li.operand.data(),
                                                       tmp_li.operand.size(), 8);
          }
          stage_leaf(tmp_li, ctx, st, lb);
          return;
        }
      }
    }


    case FilterNode::EqField:
    case FilterNode::LeField: {
      // filterEqField / filterLeField (filter_eq_field.go:122-220,
      // filter_le_field.go:155-282)
      const bool is_le = f.type == FilterNode::LeField;
      const bool excl = is_le && f.min_u != 0;
      const std::string other = canonical_field(f.min_s);
      if (li.cname == other) {
        lb.mode = excl ? kModeNone : kModeAll;
        return;
      }
      std::string cva, cvb;
      bool a_const = pr.get_const_column(ctx.bc, li.cname, &cva) && !cva.empty();
      bool b_const = pr.get_const_column(ctx.bc, other, &cvb) && !cvb.empty();
      ColumnHeader cha, chb;
      bool a_col = !a_const && pr.get_column_header(ctx.bc, li.cname, &cha);
      bool b_col = !b_const && pr.get_column_header(ctx.bc, other, &chb);
      if (a_const && b_const) {
        bool m = is_le ? le_values_string(strview(cva), strview(cvb), excl)
                       : cva == cvb;
        lb.mode = m ? kModeAll : kModeNone;
        return;
      }
      if (!a_const && !a_col && !b_const && !b_col) {
        lb.mode = excl ? kModeNone : kModeAll;  // "" vs ""
        return;
      }
      const bool same_type = a_col && b_col && cha.type == chb.type;
      lb.mode = kModeScan;
      lb.flags = excl ? 1 : 0;
      if (same_type && cha.type != ValueType::String) {
        const StagedStrCol& sa = ctx.stage_column(cha);
        const StagedStrCol& sb = ctx.stage_column(chb);
        // a staged typed column can still be const-encoded; that case falls
        // through to the generic string-form path below (decoded-string
        // compares give the same verdicts as the reference's encoded-bytes
        // compares for same-type columns; the oracle keeps the exact
        // reference logic)
        if (!sa.is_const && !sb.is_const) {
          lb.data = sa.d_data;
          lb.hashes = (const uint64_t*)sb.d_data;
          if (cha.type == ValueType::Dict) {
            // 8x8 verdict matrix over the two dicts
            uint64_t m = 0;
            for (size_t i = 0; i < cha.dict.size(); i++) {
              for (size_t j = 0; j < chb.dict.size(); j++) {
                bool v = is_le ? le_values_string(strview(cha.dict[i]),
                                                  strview(chb.dict[j]), excl)
                               : cha.dict[i] == chb.dict[j];
                if (v) m |= uint64_t(1) << (i * 8 + j);
              }
            }
            lb.kind = is_le ? kScanLeFieldDict : kScanEqFieldDict;
            lb.vmin = m;
            return;
          }
          lb.width = width_of_type(cha.type);
          if (!is_le) {
            lb.kind = kScanEqFieldBin;
            return;
          }
          if (cha.type == ValueType::Int64) {
            lb.kind = kScanLeFieldI64;
            return;
          }
          if (cha.type == ValueType::Float64) {
            lb.kind = kScanLeFieldF64;
            return;
          }
          lb.kind = kScanLeFieldBinStr;  // uint/ipv4/iso quirk path
          return;
        }
      }
      // generic string-form path: build the two side descriptors
      bytes blob(8, 0);
      bytes aux;
      auto encode_side = [&](bool isc, const std::string& cv, bool iscol,
                             const ColumnHeader& ch, int base,
                             const uint8_t*& dptr, const uint32_t*& optr) {
        dptr = nullptr;
        optr = nullptr;
        if (isc) {
          blob[base] = 1;
          blob[base + 2] = uint8_t(cv.size());
          blob[base + 3] = uint8_t(cv.size() >> 8);
          aux.insert(aux.end(), cv.begin(), cv.end());
          return;
        }
        if (!iscol) {
          blob[base] = 2;  // missing
          return;
        }
        const StagedStrCol& sc = ctx.stage_column(ch);
        if (sc.is_const) {
          // typed column encoded as const: decode its string form once
          std::string str = ch.type == ValueType::String
                                ? sc.const_value
                                : (ch.type == ValueType::Dict
                                       ? ch.dict[uint8_t(sc.const_value[0])]
                                       : format_encoded(
                                             ch.type, strview(sc.const_value)));
          blob[base] = 1;
          blob[base + 2] = uint8_t(str.size());
          blob[base + 3] = uint8_t(str.size() >> 8);
          aux.insert(aux.end(), str.begin(), str.end());
          return;
        }
        if (ch.type == ValueType::String) {
          blob[base] = 0;
          dptr = sc.d_data;
          optr = sc.d_offsets;
          return;
        }
        if (ch.type == ValueType::Dict) {
          blob[base] = 4;
          dptr = sc.d_data;
          bytes tab;
          tab.push_back(uint8_t(ch.dict.size()));
          uint16_t off = 0;
          for (size_t i = 0; i <= ch.dict.size(); i++) {
            tab.push_back(uint8_t(off));
            tab.push_back(uint8_t(off >> 8));
            if (i < ch.dict.size()) off += uint16_t(ch.dict[i].size());
          }
          for (const auto& dv : ch.dict) {
            tab.insert(tab.end(), dv.begin(), dv.end());
          }
          blob[base + 2] = uint8_t(tab.size());
          blob[base + 3] = uint8_t(tab.size() >> 8);
          aux.insert(aux.end(), tab.begin(), tab.end());
          return;
        }
        blob[base] = 3;  // formatted fixed-width
        blob[base + 1] = uint8_t(fmt_of_type(ch.type) << 4 |
                                 width_of_type(ch.type));
        dptr = sc.d_data;
      };
      const uint8_t* da;
      const uint32_t* oa;
      encode_side(a_const, cva, a_col, cha, 0, da, oa);
      size_t a_aux = aux.size();
      const uint8_t* db;
      const uint32_t* ob;
      encode_side(b_const, cvb, b_col, chb, 4, db, ob);
      (void)a_aux;
      blob.insert(blob.end(), aux.begin(), aux.end());
      lb.kind = is_le ? kScanLeFieldStr : kScanEqFieldStr;
      lb.operand = (const uint8_t*)st.push(blob.data(), blob.size(), 8);
      lb.operand_len = uint32_t(blob.size());
      lb.data = da;
      lb.offsets = oa;
      lb.hashes = (const uint64_t*)db;
      lb.bloom = (const uint64_t*)ob;
      return;
    }

    default:
      fail("stage_leaf: non-leaf node");
  }
}

// 3-valued static evaluation of the filter program over one block's staged
// leaf modes: 0 = all rows false, 1 = all rows true, 2 = needs a scan.
// Blocks whose program value is statically 0 never reach the kernel: their
// chunks are compacted out of the dispatch and their bitmap words zeroed
// once (the reference's header prunes have the same effect — e.g.
// filter_time.go:114-137 zeroes the bitmap without touching rows).  A leaf
// whose bloom gate missed at staging is kModeNone, value 0 here.
static int static_program_value(const std::vector<DevOp>& ops,
                                const DevLeafBlock* lbs) {
  std::vector<int> stack;
  stack.reserve(kMaxStackDepth + 1);
  for (const DevOp& op : ops) {
    if (op.kind == kOpLeaf) {
      const DevLeafBlock& lb = lbs[op.leaf];
      stack.push_back(lb.mode == kModeNone ? 0 : lb.mode == kModeAll ? 1 : 2);
    } else if (op.kind == kOpNot) {
      int& v = stack.back();
      if (v != 2) v = 1 - v;
    } else {
      const int n = op.nargs;
      int acc = stack[stack.size() - n];
      for (int k = 1; k < n; k++) {
        const int v = stack[stack.size() - n + k];
        if (op.kind == kOpAnd) {
          acc = (acc == 0 || v == 0) ? 0 : (acc == 1 && v == 1) ? 1 : 2;
        } else {
          acc = (acc == 1 || v == 1) ? 1 : (acc == 0 && v == 0) ? 0 : 2;
        }
      }
      stack.resize(stack.size() - n);
      stack.push_back(acc);
    }
  }
  return stack.back();
}

Stage* build_stage_refs(std::vector<std::pair<VqlPart*, long>> refs,
                        std::shared_ptr<VqlFilter> filter, int device) {
  if (refs.empty()) fail("build_stage: no blocks");
  auto st = std::make_unique<Stage>();
  st->part = refs[0].first;
  st->filter = filter;
  st->device = device;
  st->lo = 0;
  st->hi = long(refs.size());
  st->block_refs = std::move(refs);

  HIP_CHECK(hipSetDevice(device));
  // per-device: no-suffix RFC3339 parses use the host local timezone offset
  // (the reference's GetLocalTimezoneOffsetNsecs, timezone.go:9-19)
  if (vql_set_local_tz_nsecs(local_tz_offset_nsecs()) != 0) {
    fail("vql_set_local_tz_nsecs failed");
  }
  HIP_CHECK(hipStreamCreate(&st->stream));
  HIP_CHECK(hipEventCreate(&st->ev0));
  HIP_CHECK(hipEventCreate(&st->ev1));

  const long nblocks = long(st->block_refs.size());
  const int nleaves = int(filter->leaves.size());
  auto bh_of = [&](long i) -> const BlockHeader& {
    return st->block_refs[size_t(i)].first->bhs[size_t(
        st->block_refs[size_t(i)].second)];
  };

  // Device memory comes from the slab arena and grows with what is actually
  // staged (only the filter's columns), so a 1B-row part whose full column
  // set exceeds HBM still stages when the scanned columns fit.
  uint64_t rows = 0;
  for (long b = 0; b < nblocks; b++) rows += bh_of(b).rows_count;
  st->rows = rows;

  // leaf operands (block-independent)
  std::vector<LeafInfo> leaf_infos{filter->leaves.size()};
  for (size_t i = 0; i < filter->leaves.size(); i++) {
    LeafInfo& li = leaf_infos[i];
    li.node = filter->leaves[i];
    li.cname = canonical_field(li.node->field);
    switch (li.node->type) {
      case FilterNode::Phrase:
      case FilterNode::Exact:
        li.operand.assign(li.node->phrase.begin(), li.node->phrase.end());
        li.phrase_flags = phrase_flags_of(li.node->phrase);
        break;
      case FilterNode::Regexp:
        li.operand = serialize_regex(li.node->re);
        break;
      case FilterNode::Prefix:
      case FilterNode::ExactPrefix:
        li.operand.assign(li.node->phrase.begin(), li.node->phrase.end());
        li.phrase_flags = phrase_flags_of(li.node->phrase);
        break;
      case FilterNode::Sequence:
        li.operand = serialize_phrases(li.node->phrases);
        break;
      case FilterNode::In: {
        std::vector<std::string> sset = li.node->values;
        std::sort(sset.begin(), sset.end());
        sset.erase(std::unique(sset.begin(), sset.end()), sset.end());
        li.operand = serialize_str_set(sset);
        break;
      }
      case FilterNode::ContainsAll:
        li.operand = serialize_phrases(li.node->values);
        break;
      case FilterNode::StringRange: {
        bytes b;
        auto put32 = [&](uint32_t v) {
          b.push_back(uint8_t(v));
          b.push_back(uint8_t(v >> 8));
          b.push_back(uint8_t(v >> 16));
          b.push_back(uint8_t(v >> 24));
        };
        put32(uint32_t(li.node->min_s.size()));
        put32(uint32_t(li.node->max_s.size()));
        b.insert(b.end(), li.node->min_s.begin(), li.node->min_s.end());
        b.insert(b.end(), li.node->max_s.begin(), li.node->max_s.end());
        li.operand = std::move(b);
        break;
      }
      case FilterNode::DayRange:
      case FilterNode::WeekRange: {
        bytes b(8);
        int64_t off = li.node->tz_offset;
        memcpy(b.data(), &off, 8);
        li.operand = std::move(b);
        break;
      }
      case FilterNode::AnyCasePhrase:
      case FilterNode::AnyCasePrefix:
        li.operand.assign(li.node->min_s.begin(), li.node->min_s.end());
        li.phrase_flags = phrase_flags_of(li.node->min_s);
        break;
      default:
        break;
    }
    if (!li.operand.empty()) {
      li.d_operand = st->push(li.operand.data(), li.operand.size(), 8);
    }
  }

  // bitmap output buffer
  st->block_word_off.resize(size_t(nblocks) + 1, 0);
  for (long b = 0; b < nblocks; b++) {
    st->block_word_off[size_t(b) + 1] =
        st->block_word_off[size_t(b)] + (bh_of(b).rows_count + 63) / 64;
  }
  st->bitmap_words = size_t(st->block_word_off.back());
  st->d_bitmap = (uint64_t*)st->reserve(st->bitmap_words * 8, 8);

  // per-block staging
  std::vector<DevBlock> blocks_h((size_t(nblocks)));
  std::vector<DevLeafBlock> lbs_h(size_t(nblocks) * size_t(nleaves));
  std::vector<DevChunk> chunks_h;
  for (long b = 0; b < nblocks; b++) {
    VqlPart* bp = st->block_refs[size_t(b)].first;
    const BlockHeader& bh = bh_of(b);
    BlockStageCtx ctx;
    ctx.st = st.get();
    ctx.pr = &bp->pr;
    ctx.bh = &bh;
    bp->pr.read_block_columns(bh, ctx.bc);

    DevBlock& db = blocks_h[size_t(b)];
    db.rows = uint32_t(bh.rows_count);
    db.bitmap_out = st->d_bitmap + st->block_word_off[size_t(b)];
    db.hits_out = nullptr;  // filled after d_block_hits is allocated

    // watermark: if the block is statically eliminated below, its staged
    // column data is reclaimed (bump-allocator rollback)
    const Stage::ArenaMark arena_mark = st->mark();
    uint64_t block_algo = 0;

    for (int l = 0; l < nleaves; l++) {
      DevLeafBlock& lb = lbs_h[size_t(b) * size_t(nleaves) + size_t(l)];
      stage_leaf(leaf_infos[size_t(l)], ctx, *st, lb);
      if (lb.mode == kModeScan) {
        // algorithmic bytes one pass must read for this leaf
        switch (lb.kind) {
          case kScanPhraseStr:
          case kScanEqStr:
          case kScanRegexStr:
          case kScanRangeStr:
          case kScanPrefixStr:
          case kScanExactPrefixStr:
          case kScanSeqStr:
          case kScanInStr:
          case kScanAnyPhraseStr:
          case kScanAllPhrasesStr:
          case kScanStrRange:
          case kScanIPv4RangeStr:
          case kScanLenRangeStr:
          case kScanAnyCasePhraseStr:
          case kScanAnyCasePrefixStr: {
            const StagedStrCol& sc = ctx.cols.at(leaf_infos[size_t(l)].cname);
            block_algo += sc.data_bytes + (bh.rows_count + 1) * 4;
            // small-row super-group size, from the block's actual spans
            if (sc.rows > 0) lb.sg = sc.sg;
            break;
          }
          case kScanDict:
            block_algo += bh.rows_count;
            break;
          case kScanTsRange:
            block_algo += bh.rows_count * 8;
            break;
          default:
            block_algo += bh.rows_count * (lb.width ? lb.width : 8);
            break;
        }
      }
    }

    if (static_program_value(filter->ops,
                             &lbs_h[size_t(b) * size_t(nleaves)]) == 0) {
      // statically all-zero result: no chunks dispatched, bitmap words zeroed
      // once at the first scan, staged column data reclaimed
      st->rollback(arena_mark);
      const uint64_t w0 = st->block_word_off[size_t(b)];
      const uint64_t w1 = st->block_word_off[size_t(b) + 1];
      if (!st->zero_word_ranges.empty() &&
          st->zero_word_ranges.back().second == w0) {
        st->zero_word_ranges.back().second = w1;
      } else {
        st->zero_word_ranges.emplace_back(w0, w1);
      }
      continue;
    }
    st->algo_bytes += block_algo;
    st->live_rows += bh.rows_count;
    // bitmap write traffic for this (live) block
    st->algo_bytes +=
        (st->block_word_off[size_t(b) + 1] - st->block_word_off[size_t(b)]) * 8;
    // chunks
    uint32_t nch = uint32_t((bh.rows_count + kChunkRows - 1) / kChunkRows);
    for (uint32_t c = 0; c < nch; c++) {
      chunks_h.push_back(DevChunk{uint32_t(b), c});
    }
  }

  st->nchunks = uint32_t(chunks_h.size());
  st->chunks_h = chunks_h;
  for (long b = 0; b < nblocks; b++) {
    st->block_rows_h.push_back(uint32_t(bh_of(b).rows_count));
  }

  HIP_CHECK(hipMalloc(&st->d_ops, filter->ops.size() * sizeof(DevOp)));
  HIP_CHECK(hipMemcpy(st->d_ops, filter->ops.data(),
                      filter->ops.size() * sizeof(DevOp), hipMemcpyHostToDevice));
  HIP_CHECK(hipMalloc(&st->d_lbs, lbs_h.size() * sizeof(DevLeafBlock)));
  HIP_CHECK(hipMemcpy(st->d_lbs, lbs_h.data(), lbs_h.size() * sizeof(DevLeafBlock),
                      hipMemcpyHostToDevice));
  HIP_CHECK(hipMalloc(&st->d_block_hits, size_t(nblocks) * 8));
  for (long b = 0; b < nblocks; b++) {
    blocks_h[size_t(b)].hits_out = st->d_block_hits + b;
  }
  HIP_CHECK(hipMalloc(&st->d_blocks, blocks_h.size() * sizeof(DevBlock)));
  HIP_CHECK(hipMemcpy(st->d_blocks, blocks_h.data(),
                      blocks_h.size() * sizeof(DevBlock), hipMemcpyHostToDevice));
  if (!chunks_h.empty()) {
    HIP_CHECK(hipMalloc(&st->d_chunks, chunks_h.size() * sizeof(DevChunk)));
    HIP_CHECK(hipMemcpy(st->d_chunks, chunks_h.data(),
                        chunks_h.size() * sizeof(DevChunk),
                        hipMemcpyHostToDevice));
  }
  HIP_CHECK(hipMalloc(&st->d_hits, 8));

  return st.release();
}

Stage* build_stage(VqlPart* part, std::shared_ptr<VqlFilter> filter, int device,
                   long lo, long hi) {
  if (hi < 0 || size_t(hi) > part->bhs.size()) hi = long(part->bhs.size());
  if (lo < 0) lo = 0;
  std::vector<std::pair<VqlPart*, long>> refs;
  refs.reserve(size_t(hi - lo));
  for (long b = lo; b < hi; b++) refs.emplace_back(part, b);
  Stage* st = build_stage_refs(std::move(refs), std::move(filter), device);
  st->lo = lo;
  st->hi = hi;
  return st;
}

long long run_scan(Stage* st) {
  HIP_CHECK(hipSetDevice(st->device));
  HIP_CHECK(hipMemsetAsync(st->d_hits, 0, 8, st->stream));
  HIP_CHECK(hipMemsetAsync(st->d_block_hits, 0,
                           st->block_refs.size() * 8, st->stream));
  if (!st->bitmap_zeroed) {
    // statically-eliminated blocks never reach the kernel; their bitmap
    // words are zeroed once (they stay zero — live blocks rewrite their own
    // words every scan)
    for (const auto& r : st->zero_word_ranges) {
      HIP_CHECK(hipMemsetAsync(st->d_bitmap + r.first, 0,
                               (r.second - r.first) * 8, st->stream));
    }
    st->bitmap_zeroed = true;
  }
  HIP_CHECK(hipEventRecord(st->ev0, st->stream));
  HIP_CHECK(vql_launch_scan(st->d_ops, int(st->filter->ops.size()), st->d_lbs,
                            int(st->filter->leaves.size()), st->d_blocks,
                            st->d_chunks, st->nchunks, st->d_hits, st->stream));
  HIP_CHECK(hipEventRecord(st->ev1, st->stream));
  unsigned long long hits = 0;
  HIP_CHECK(hipMemcpyAsync(&hits, st->d_hits, 8, hipMemcpyDeviceToHost, st->stream));
  HIP_CHECK(hipStreamSynchronize(st->stream));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, st->ev0, st->ev1));
  st->last_kernel_ms = double(ms);
  return (long long)hits;
}

}  // namespace

extern "C" {

const char* vql_errstr() { return g_err.c_str(); }

/* 1 if the last error on this thread was an unsupported-construct
 * rejection (a valid LogsQL filter outside the engine's class — e.g. a
 * regex using \p{...}) rather than corruption/IO.  A drop-in shim
 * routes such filters back to the host's own Go implementation
 * (INTEGRATION.md "Unsupported-filter fallback"); corruption errors keep
 * the reference's panic semantics. */
int vql_error_unsupported(void) {
  return g_err.compare(0, 7, "regex: ") == 0 ? 1 : 0;
}

void* vql_open_part(const char* dir) {
  try {
    return new VqlPart(dir);
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void vql_close_part(void* p) { delete (VqlPart*)p; }
long vql_part_blocks(void* p) { return long(((VqlPart*)p)->bhs.size()); }
long long vql_part_rows(void* p) {
  return (long long)((VqlPart*)p)->pr.header().rows_count;
}
long vql_block_rows(void* p, long i) {
  return long(((VqlPart*)p)->bhs[size_t(i)].rows_count);
}

void* vql_compile_filter(const char* json) {
  try {
    return new std::shared_ptr<VqlFilter>(
        std::make_shared<VqlFilter>(compile_filter(json)));
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void vql_free_filter(void* f) { delete (std::shared_ptr<VqlFilter>*)f; }

void* vql_stage(void* part, void* filter, int device, long block_lo, long block_hi) {
  try {
    return build_stage((VqlPart*)part, *(std::shared_ptr<VqlFilter>*)filter, device,
                       block_lo, block_hi);
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}

/* Stages ALL blocks of `nparts` parts into one context: one kernel launch
 * scans everything (the reference batches blocks regardless of their part,
 * storage_search.go:1035-1067). */
void* vql_stage_parts(void** parts, int nparts, void* filter, int device) {
  try {
    std::vector<std::pair<VqlPart*, long>> refs;
    for (int i = 0; i < nparts; i++) {
      auto* p = (VqlPart*)parts[i];
      for (long b = 0; b < long(p->bhs.size()); b++) refs.emplace_back(p, b);
    }
    return build_stage_refs(std::move(refs),
                            *(std::shared_ptr<VqlFilter>*)filter, device);
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
void vql_stage_free(void* s) { delete (Stage*)s; }
long long vql_stage_bytes(void* s) { return (long long)((Stage*)s)->staged_bytes; }
long long vql_stage_algo_bytes(void* s) {
  return (long long)((Stage*)s)->algo_bytes;
}
long long vql_stage_rows(void* s) { return (long long)((Stage*)s)->rows; }
long long vql_stage_live_rows(void* s) {
  return (long long)((Stage*)s)->live_rows;
}

long long vql_scan_staged(void* s) {
  try {
    return run_scan((Stage*)s);
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

double vql_last_kernel_ms(void* s) { return ((Stage*)s)->last_kernel_ms; }

// Copies the result bitmaps (concatenated per-block words, same layout as
// the oracle's orc_scan_blocks) to out_words.  Returns 0, or -1 on error.
int vql_fetch_bitmaps(void* s, unsigned long long* out_words, long long cap) {
  try {
    Stage* st = (Stage*)s;
    if ((long long)st->bitmap_words > cap) fail("vql_fetch_bitmaps: buffer too small");
    HIP_CHECK(hipSetDevice(st->device));
    HIP_CHECK(hipMemcpy(out_words, st->d_bitmap, st->bitmap_words * 8,
                        hipMemcpyDeviceToHost));
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// Per-block matched-row counts of the last vql_scan_staged -- the
// blockResult rowsLen popcount (block_result.go:403-413) and the
// `| stats count()` fast path.  Returns 0 or -1.
int vql_fetch_block_hits(void* s, unsigned long long* out, long long cap) {
  try {
    Stage* st = (Stage*)s;
    long n = long(st->block_refs.size());
    if (cap < n) fail("vql_fetch_block_hits: buffer too small");
    HIP_CHECK(hipSetDevice(st->device));
    HIP_CHECK(hipMemcpy(out, st->d_block_hits, size_t(n) * 8,
                        hipMemcpyDeviceToHost));
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// Cold path (SURVEY.md §8b vql_scan_batch): stage blocks [lo,hi), scan once,
// fetch bitmaps, free.  Returns matched rows or -1.
// Whole-query driver (SURVEY.md §8b vql_scan_query): parts round-robin over
// devices, one staging+scan thread per device, counters summed in-process.
struct VqlStatsC {
  unsigned long long matched_rows;
  unsigned long long rows_scanned;
  unsigned long long bytes_scanned;
  double elapsed_ms;
};

extern "C" long long vql_scan_query(void** parts, int nparts, void* filter,
                                    int ngpus, VqlStatsC* stats) {
  try {
    if (nparts <= 0 || ngpus <= 0) fail("vql_scan_query: bad arguments");
    auto& vf = *(std::shared_ptr<VqlFilter>*)filter;
    std::vector<std::thread> threads;
    std::vector<unsigned long long> hits(size_t(ngpus), 0);
    std::vector<unsigned long long> rows(size_t(ngpus), 0);
    std::vector<unsigned long long> bytes(size_t(ngpus), 0);
    std::vector<std::string> errs{std::vector<std::string>::size_type(ngpus)};
    auto t0 = std::chrono::steady_clock::now();
    for (int d = 0; d < ngpus; d++) {
      threads.emplace_back([&, d]() {
        try {
          std::vector<std::pair<VqlPart*, long>> refs;
          for (int i = d; i < nparts; i += ngpus) {
            auto* p = (VqlPart*)parts[i];
            for (long b = 0; b < long(p->bhs.size()); b++) {
              refs.emplace_back(p, b);
            }
          }
          if (!refs.empty()) {
            Stage* st = build_stage_refs(std::move(refs), vf, d);
            std::unique_ptr<Stage> guard(st);
            long long h2 = run_scan(st);
            if (h2 < 0) fail("scan failed");
            hits[size_t(d)] += (unsigned long long)h2;
            rows[size_t(d)] += st->rows;
            bytes[size_t(d)] += st->algo_bytes;
          }
        } catch (const std::exception& e) {
          errs[size_t(d)] = e.what();
        }
      });
    }
    for (auto& t : threads) t.join();
    for (const auto& e : errs) {
      if (!e.empty()) fail("vql_scan_query: " + e);
    }
    double ms = std::chrono::duration<double, std::milli>(
                    std::chrono::steady_clock::now() - t0)
                    .count();
    unsigned long long h = 0, r = 0, b = 0;
    for (int d = 0; d < ngpus; d++) {
      h += hits[size_t(d)];
      r += rows[size_t(d)];
      b += bytes[size_t(d)];
    }
    if (stats) {
      stats->matched_rows = h;
      stats->rows_scanned = r;
      stats->bytes_scanned = b;
      stats->elapsed_ms = ms;
    }
    return (long long)h;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// GPU ingest-side bloom build: marshaled bloom bytes
// for one column block, bit-identical to the write path's
// tokenizeHashes + bloomFilterMarshalHashes (block.go:160-168).  `offsets` is
// u32[rows+1] over the concatenated value bytes.  Returns the marshaled
// length (BE u64 words); fills `out` when cap suffices; -1 on error.
extern "C" int vql_launch_bloom_tokenize(const void*, const void*, unsigned,
                                         void*, unsigned, void*, void*, void*);
extern "C" int vql_launch_bloom_setbits(const void*, unsigned, void*,
                                        unsigned long long, void*);

extern "C" long long vql_bloom_build(const unsigned char* data,
                                     long long nbytes,
                                     const unsigned int* offsets,
                                     long long rows, int device,
                                     unsigned char* out, long long cap) {
  try {
    HIP_CHECK(hipSetDevice(device));
    uint8_t* d_data = nullptr;
    uint32_t* d_offs = nullptr;
    unsigned long long* d_slots = nullptr;
    unsigned long long* d_unique = nullptr;
    int* d_overflow = nullptr;
    uint64_t* d_bits = nullptr;
    auto cleanup = [&]() {
      if (d_data) (void)hipFree(d_data);
      if (d_offs) (void)hipFree(d_offs);
      if (d_slots) (void)hipFree(d_slots);
      if (d_unique) (void)hipFree(d_unique);
      if (d_overflow) (void)hipFree(d_overflow);
      if (d_bits) (void)hipFree(d_bits);
    };
    HIP_CHECK(hipMalloc(&d_data, size_t(nbytes) + 16));
    HIP_CHECK(hipMemcpy(d_data, data, size_t(nbytes), hipMemcpyHostToDevice));
    HIP_CHECK(hipMalloc(&d_offs, (size_t(rows) + 1) * 4));
    HIP_CHECK(hipMemcpy(d_offs, offsets, (size_t(rows) + 1) * 4,
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMalloc(&d_unique, 8));
    HIP_CHECK(hipMalloc(&d_overflow, 4));

    uint64_t cap_slots = 1024;
    while (cap_slots < uint64_t(nbytes) / 2 + 1024) cap_slots <<= 1;
    // start smaller for realistic corpora; grow on overflow
    uint64_t try_cap = 1 << 16;
    unsigned long long unique = 0;
    for (;;) {
      if (try_cap > cap_slots) try_cap = cap_slots;
      HIP_CHECK(hipMalloc(&d_slots, try_cap * 8));
      HIP_CHECK(hipMemset(d_slots, 0, try_cap * 8));
      HIP_CHECK(hipMemset(d_unique, 0, 8));
      HIP_CHECK(hipMemset(d_overflow, 0, 4));
      if (vql_launch_bloom_tokenize(d_data, d_offs, unsigned(rows), d_slots,
                                    unsigned(try_cap - 1), d_unique,
                                    d_overflow, nullptr) != 0) {
        cleanup();
        fail("bloom tokenize launch failed");
      }
      int overflow = 0;
      HIP_CHECK(hipMemcpy(&overflow, d_overflow, 4, hipMemcpyDeviceToHost));
      HIP_CHECK(hipMemcpy(&unique, d_unique, 8, hipMemcpyDeviceToHost));
      // keep the table below half full so dedup probing stays short
      if (!overflow && unique * 2 <= try_cap) break;
      (void)hipFree(d_slots);
      d_slots = nullptr;
      if (try_cap >= cap_slots) {
        cleanup();
        fail("bloom hash set overflow");
      }
      try_cap <<= 2;
    }
    const uint64_t bits_count = unique * 16;  // bloomFilterBitsPerItem
    const uint64_t words = (bits_count + 63) / 64;
    const long long out_len = (long long)(words * 8);
    if (words > 0 && out_len <= cap) {
      HIP_CHECK(hipMalloc(&d_bits, words * 8));
      HIP_CHECK(hipMemset(d_bits, 0, words * 8));
      if (vql_launch_bloom_setbits(d_slots, unsigned(try_cap), d_bits,
                                   words * 64, nullptr) != 0) {
        cleanup();
        fail("bloom setbits launch failed");
      }
      std::vector<uint64_t> host_words(words);
      HIP_CHECK(hipMemcpy(host_words.data(), d_bits, words * 8,
                          hipMemcpyDeviceToHost));
      for (uint64_t i = 0; i < words; i++) {
        uint64_t w = host_words[i];
        for (int b = 7; b >= 0; b--) {
          out[i * 8 + (7 - b)] = uint8_t(w >> (b * 8));  // BE marshal
        }
      }
    }
    cleanup();
    return out_len;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

long long vql_scan_batch(void* part, void* filter, long lo, long hi,
                         unsigned long long* out_words, long long cap,
                         unsigned long long* out_popcounts) {
  void* st = vql_stage(part, filter, 0, lo, hi);
  if (!st) return -1;
  long long hits = vql_scan_staged(st);
  if (hits >= 0 && out_words) {
    if (vql_fetch_bitmaps(st, out_words, cap) != 0) hits = -1;
  }
  if (hits >= 0 && out_popcounts) {
    long n = hi < 0 ? vql_part_blocks(part) : hi;
    if (vql_fetch_block_hits(st, out_popcounts, n - (lo < 0 ? 0 : lo)) != 0) {
      hits = -1;
    }
  }
  vql_stage_free(st);
  return hits;
}

}  // extern "C"

namespace {

// Builds (and caches) the per-block gather descriptors for `field` and runs
// the count pass.  Mirrors blockResult.getValues source selection
// (block_result.go:306-478): const columns repeat the const value, dict
// columns look up the dict string, fixed-width columns decode to strings.
Stage::GatherCtx& gather_prepare(Stage* st, const std::string& field) {
  auto it = st->gathers.find(field);
  if (it != st->gathers.end() && it->second.sized) return it->second;

  HIP_CHECK(hipSetDevice(st->device));
  Stage::GatherCtx& g = st->gathers[field];
  std::string cname = canonical_field(field);
  const long nblocks = long(st->block_refs.size());

  std::vector<DevGatherCol> gcols((size_t(nblocks)));
  for (long b = 0; b < nblocks; b++) {
    VqlPart* bpart = st->block_refs[size_t(b)].first;
    const BlockHeader& bh =
        bpart->bhs[size_t(st->block_refs[size_t(b)].second)];
    PartReader::BlockColumns bc;
    bpart->pr.read_block_columns(bh, bc);
    DevGatherCol& gc = gcols[size_t(b)];
    memset(&gc, 0, sizeof(gc));

    std::string cv;
    if (bpart->pr.get_const_column(bc, cname, &cv)) {
      gc.src = kGatherConst;
      gc.cval_len = uint32_t(cv.size());
      gc.cval = st->push(cv.data(), cv.size(), 8);
      continue;
    }
    ColumnHeader ch;
    if (!bpart->pr.get_column_header(bc, cname, &ch)) {
      gc.src = kGatherMissing;
      continue;
    }
    StringsBlockDec dec;
    bpart->pr.read_values(ch, bh.rows_count, dec);
    if (dec.is_const && ch.type == ValueType::String) {
      gc.src = kGatherConst;
      gc.cval_len = uint32_t(dec.data.size());
      gc.cval = st->push(dec.data.data(), dec.data.size(), 8);
      continue;
    }
    // non-const data payload
    const uint8_t* d_data = st->push(dec.data.data(), dec.data.size(), 16);
    st->reserve(16);
    gc.data = d_data;
    switch (ch.type) {
      case ValueType::String: {
        gc.src = kGatherStr;
        gc.offsets = (const uint32_t*)st->push(dec.offsets.data(),
                                               dec.offsets.size() * 4, 4);
        break;
      }
      case ValueType::Dict: {
        gc.src = kGatherDict;
        bytes cat;
        std::vector<uint32_t> doffs;
        doffs.push_back(0);
        for (const auto& dv : ch.dict) {
          cat.insert(cat.end(), dv.begin(), dv.end());
          doffs.push_back(uint32_t(cat.size()));
        }
        while (doffs.size() < 9) doffs.push_back(doffs.back());
        gc.dict_data = st->push(cat.data(), cat.size(), 8);
        gc.dict_offs = (const uint32_t*)st->push(doffs.data(), doffs.size() * 4, 4);
        break;
      }
      case ValueType::Uint8: gc.src = kGatherFmtU; gc.width = 1; break;
      case ValueType::Uint16: gc.src = kGatherFmtU; gc.width = 2; break;
      case ValueType::Uint32: gc.src = kGatherFmtU; gc.width = 4; break;
      case ValueType::Uint64: gc.src = kGatherFmtU; gc.width = 8; break;
      case ValueType::Int64: gc.src = kGatherFmtI; gc.width = 8; break;
      case ValueType::Float64: gc.src = kGatherFmtF; gc.width = 8; break;
      case ValueType::IPv4: gc.src = kGatherFmtIp; gc.width = 4; break;
      case ValueType::TimestampISO8601: gc.src = kGatherFmtIso; gc.width = 8; break;
      default:
        fail("gather: unknown valueType");
    }
  }
  HIP_CHECK(hipMalloc(&g.d_gcols, gcols.size() * sizeof(DevGatherCol)));
  HIP_CHECK(hipMemcpy(g.d_gcols, gcols.data(), gcols.size() * sizeof(DevGatherCol),
                      hipMemcpyHostToDevice));

  // count pass
  DevChunkCount* d_counts = nullptr;
  HIP_CHECK(hipMalloc(&d_counts, st->nchunks * sizeof(DevChunkCount)));
  HIP_CHECK(vql_launch_gather_count(g.d_gcols, st->d_blocks, st->d_chunks,
                                    st->nchunks, d_counts, st->stream));
  std::vector<DevChunkCount> counts(st->nchunks);
  HIP_CHECK(hipMemcpyAsync(counts.data(), d_counts,
                           st->nchunks * sizeof(DevChunkCount),
                           hipMemcpyDeviceToHost, st->stream));
  HIP_CHECK(hipStreamSynchronize(st->stream));
  HIP_CHECK(hipFree(d_counts));

  // exclusive scan -> per-chunk bases; gid_base = first global row of block
  std::vector<unsigned long long> block_row_base(st->block_refs.size() + 1, 0);
  for (size_t b = 0; b < st->block_rows_h.size(); b++) {
    block_row_base[b + 1] = block_row_base[b] + st->block_rows_h[b];
  }
  std::vector<DevChunkBase> bases(st->nchunks);
  unsigned long long racc = 0, bacc = 0;
  for (uint32_t c = 0; c < st->nchunks; c++) {
    bases[c].row_base = racc;
    bases[c].byte_base = bacc;
    bases[c].gid_base = block_row_base[st->chunks_h[c].block];
    racc += counts[c].rows;
    bacc += counts[c].bytes;
  }
  g.nrows = racc;
  g.nbytes = bacc;
  HIP_CHECK(hipMalloc(&g.d_bases, bases.size() * sizeof(DevChunkBase)));
  HIP_CHECK(hipMemcpy(g.d_bases, bases.data(), bases.size() * sizeof(DevChunkBase),
                      hipMemcpyHostToDevice));
  g.sized = true;
  return g;
}

}  // namespace

extern "C" {

// Sizes of the gather output for `field` over the CURRENT bitmaps (run a scan
// first).  Returns 0 or -1.
int vql_gather_sizes(void* s, const char* field, unsigned long long* nrows,
                     unsigned long long* nbytes) {
  try {
    Stage* st = (Stage*)s;
    Stage::GatherCtx& g = gather_prepare(st, field);
    *nrows = g.nrows;
    *nbytes = g.nbytes;
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

// Gathers the matched rows' values of `field` into packed bytes (out_bytes),
// per-row byte offsets (out_offs, nrows+1 entries) and optional global row
// ids (out_rowids, nrows entries).  Returns the matched-row count or -1.
long long vql_gather(void* s, const char* field, unsigned char* out_bytes,
                     long long bytes_cap, unsigned long long* out_offs,
                     long long offs_cap, unsigned long long* out_rowids) {
  try {
    Stage* st = (Stage*)s;
    Stage::GatherCtx& g = gather_prepare(st, field);
    if ((long long)g.nbytes > bytes_cap) fail("vql_gather: bytes buffer too small");
    if ((long long)(g.nrows + 1) > offs_cap) fail("vql_gather: offsets buffer too small");
    HIP_CHECK(hipSetDevice(st->device));
    uint8_t* d_bytes = nullptr;
    unsigned long long* d_offs = nullptr;
    unsigned long long* d_rowids = nullptr;
    HIP_CHECK(hipMalloc(&d_bytes, g.nbytes ? g.nbytes : 8));
    HIP_CHECK(hipMalloc(&d_offs, (g.nrows + 1) * 8));
    if (out_rowids) HIP_CHECK(hipMalloc(&d_rowids, g.nrows ? g.nrows * 8 : 8));
    HIP_CHECK(vql_launch_gather_copy(g.d_gcols, st->d_blocks, st->d_chunks,
                                     st->nchunks, g.d_bases, d_bytes, d_offs,
                                     d_rowids, st->stream));
    HIP_CHECK(hipStreamSynchronize(st->stream));
    if (g.nbytes) {
      HIP_CHECK(hipMemcpy(out_bytes, d_bytes, g.nbytes, hipMemcpyDeviceToHost));
    }
    HIP_CHECK(hipMemcpy(out_offs, d_offs, g.nrows * 8, hipMemcpyDeviceToHost));
    out_offs[g.nrows] = g.nbytes;
    if (out_rowids && g.nrows) {
      HIP_CHECK(hipMemcpy(out_rowids, d_rowids, g.nrows * 8, hipMemcpyDeviceToHost));
    }
    (void)hipFree(d_bytes);
    (void)hipFree(d_offs);
    if (d_rowids) (void)hipFree(d_rowids);
    return (long long)g.nrows;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  }
}

}  // extern "C"
