// scan_plan.cpp -- the steps the bitmap-then-scan plans share (scan_plan.h).
#include "scan_plan.h"

#include <algorithm>
#include <cstring>

namespace ph {

void check_query(const ph_query* q) {
  if (!q) fail(PH_ERR_INVALID_ARGUMENT, "null query");
  if (q->num_aggregations < 0 || (q->num_aggregations > 0 && !q->aggregations))
    fail(PH_ERR_INVALID_ARGUMENT, "bad aggregation list");
}

void refuse_plain_beside(const Family& f, const ph_aggregation& a) {
  if (a.type < PH_AGG_SUM || a.type > PH_AGG_PERCENTILE) return;
  static const char* fn[] = {"SUM", "MIN", "MAX", "DISTINCTCOUNTHLL", "DISTINCTCOUNT", "PERCENTILE"};
  fail(PH_ERR_UNSUPPORTED, std::string(fn[a.type - PH_AGG_SUM]) + " beside a " + f.word + " function");
}

void check_shape(const Family& f, const ph_query* q) {
  if (q->num_aggregations > kMaxAggs) fail(PH_ERR_UNSUPPORTED, "too many aggregations");
  if (q->num_group_by > kMaxGroupCols) fail(PH_ERR_UNSUPPORTED, "too many group-by columns");
  if (q->min_segment_group_trim_size > 0 && q->num_group_by > 0 && q->num_order_by > 0)
    fail(PH_ERR_UNSUPPORTED, std::string(f.plural) + " with segment group trim (minSegmentGroupTrimSize)");
}

void check_interrupt(const ph_query* q) {
  if (q->interrupt && *q->interrupt) fail(PH_ERR_CANCELLED, "query interrupted");
}

void check_deadline(const ph_query* q) {
  if (q->end_time_ms <= 0) return;
  const int64_t now = std::chrono::duration_cast<std::chrono::milliseconds>(
                          std::chrono::system_clock::now().time_since_epoch()).count();
  if (now > q->end_time_ms) fail(PH_ERR_CANCELLED, "query timed out (end time passed)");
}

std::vector<ph_segment*> check_call(Context* ctx, const ph_query* q, ph_segment* const* segs_in, int32_t nseg) {
  if (nseg < 0 || (nseg > 0 && !segs_in)) fail(PH_ERR_INVALID_ARGUMENT, "bad segment list");
  std::vector<ph_segment*> segs(segs_in, segs_in + nseg);
  for (auto* s : segs)
    if (!s || s->ctx != ctx) fail(PH_ERR_INVALID_ARGUMENT, "segment is null or pinned on another context");
  check_interrupt(q);
  check_deadline(q);
  return segs;
}

std::vector<std::string> group_columns(const ph_query* q) {
  std::vector<std::string> group_cols;
  for (int g = 0; g < q->num_group_by; ++g) {
    if (!q->group_by || !q->group_by[g]) fail(PH_ERR_INVALID_ARGUMENT, "null group-by column");
    group_cols.push_back(q->group_by[g]);
  }
  return group_cols;
}

static const std::string kNotFound = "Column not found: ";

const Column& column_in(const ph_segment* seg, const std::string& col) {
  auto it = seg->columns.find(col);
  if (it == seg->columns.end()) fail(PH_ERR_BAD_QUERY, kNotFound + col + " in segment " + seg->name);
  return *it->second;
}

void check_columns(const ph_query* q, const std::vector<ph_segment*>& segs, const std::vector<std::string>& group_cols) {
  for (auto* s : segs) {
    for (auto& c : group_cols) column_in(s, c);
    for (int i = 0; i < q->num_predicates; ++i) {
      if (!q->predicates[i].column) fail(PH_ERR_BAD_QUERY, "predicate without column");
      if (!s->columns.count(q->predicates[i].column))
        fail(PH_ERR_BAD_QUERY, kNotFound + q->predicates[i].column);
    }
  }
}

NumericRange numeric_range(const Family& f, const std::string& col, const std::vector<ph_segment*>& segs) {
  NumericRange r;
  const std::string word = f.word;
  int col_int = -1;
  for (auto* seg : segs) {
    const Column& c = column_in(seg, col);
    if (c.data_type == PH_STRING) fail(PH_ERR_UNSUPPORTED, word + " function on STRING column " + col);
    if (c.sketch_words) fail(PH_ERR_UNSUPPORTED, word + " function on sketch column " + col);
    const int ci = c.data_type == PH_INT || c.data_type == PH_LONG;
    if (col_int < 0) col_int = ci;
    else if (col_int != ci) fail(PH_ERR_UNSUPPORTED, word + " column with mixed integer/real types across segments");
    if (c.cardinality <= 0) continue;
    if (ci) {
      r.ilo = r.any ? std::min(r.ilo, c.dict.ints.front()) : c.dict.ints.front();
      r.ihi = r.any ? std::max(r.ihi, c.dict.ints.back()) : c.dict.ints.back();
    } else {
      r.lo = r.any ? std::min(r.lo, c.dict.reals.front()) : c.dict.reals.front();
      r.hi = r.any ? std::max(r.hi, c.dict.reals.back()) : c.dict.reals.back();
    }
    r.any = true;
  }
  r.is_int = col_int != 0;
  if (r.is_int) {
    r.lo = (double)r.ilo;
    r.hi = (double)r.ihi;
  }
  return r;
}

int32_t where_class(const ph_query* q, ph_segment* seg) {
  if (q->filter_root >= 0) return filter_plan_class(q, q->filter_root, seg);
  return seg->num_docs == 0 ? FP_EMPTY : FP_ALL;
}

WhereBitmap where_bitmap(Context* ctx, const ph_query* q, int32_t root, ph_segment* seg, Scratch& scratch, double& dev_ms) {
  WhereBitmap b;
  const int64_t need = std::max<int64_t>(1, ((int64_t)seg->num_docs + 63) / 64);
  b.words = scratch.alloc<unsigned long long>((size_t)need);
  ph_query qc = *q;
  ph_aggregation cnt{};
  cnt.type = PH_AGG_COUNT;
  qc.filter_root = root;
  qc.num_group_by = 0;
  qc.group_by = nullptr;
  qc.num_aggregations = 1;
  qc.aggregations = &cnt;
  qc.num_order_by = 0;
  qc.order_by = nullptr;
  qc.min_segment_group_trim_size = -1;
  qc.skip_star_tree = 1;
  qc.histograms = nullptr;
  qc.with_time = nullptr;
  const int64_t off[1] = {0};
  FilterDocset fd{b.words, off, need};
  DenseArgs d{0, nullptr, 0, 0, nullptr};
  d.docset = &fd;
  ph_segment* one[1] = {seg};
  std::unique_ptr<ph_result> r(query_execute_impl(ctx, &qc, one, 1, &d));  // drains its stream before it returns
  b.docs = r->stats.num_docs_scanned;
  b.entries = r->stats.num_entries_scanned_in_filter;
  dev_ms += r->stats.device_ms;
  return b;
}

KeySpace key_space(const Family& f, const std::vector<std::string>& group_cols, const std::vector<ph_segment*>& segs) {
  KeySpace ks;
  ks.group_cols = group_cols;
  for (auto& g : group_cols) {
    if (segs.empty()) fail(PH_ERR_UNSUPPORTED, std::string(f.word) + " group-by without segments");
    ks.gdicts.push_back(union_dictionary(g, segs));
    const int64_t sz = ks.size(ks.gdicts.size() - 1);
    if (ks.G > (int64_t(1) << 40) / sz)
      fail(PH_ERR_UNSUPPORTED, std::string(f.plural) + " over a group key space beyond the dense tables");
    ks.G *= sz;
  }
  int64_t stride = 1;
  for (int g = (int)group_cols.size() - 1; g >= 0; --g) {
    ks.stride[g] = stride;
    stride *= ks.size((size_t)g);
  }
  return ks;
}

void refuse_group_limit(const Family& f, const ph_query* q, const KeySpace& ks, const std::vector<ph_segment*>& segs,
                        const std::vector<int32_t>& cls) {
  if (ks.group_cols.empty()) return;
  const int64_t group_limit = q->num_groups_limit > 0 ? q->num_groups_limit : 100000;
  for (size_t i = 0; i < segs.size(); ++i) {
    if (cls[i] == FP_EMPTY) continue;
    int64_t pp = 1;
    for (auto& g : ks.group_cols) {
      const int64_t c = std::max<int64_t>(1, segs[i]->columns.at(g)->cardinality);
      pp = pp > (int64_t(1) << 40) / c ? int64_t(1) << 40 : pp * c;
    }
    // past the limit the groups the reference keeps depend on the order it meets them in (and, with FILTER clauses, on
    // the order of a HashMap over FilterContexts)
    if (std::min<int64_t>(pp, segs[i]->num_docs) >= group_limit)
      fail(PH_ERR_UNSUPPORTED, std::string(f.plural) + " where a segment could reach numGroupsLimit");
  }
}

int choose_mode(Context* ctx, const Family& f, const KeySpace& ks, double table_bytes, double lds_bytes) {
  if (table_bytes > kDenseTableBudget)
    fail(PH_ERR_UNSUPPORTED, std::string(f.plural) + " over a group key space beyond the dense tables");
  if (ks.group_cols.empty()) return MODE_AGG;
  size_t lds_table_max = 64 * 1024;
  if (ctx->has(OPT_LDS_TABLE_MAX)) lds_table_max = (size_t)std::max<int64_t>(0, ctx->opt(OPT_LDS_TABLE_MAX));
  lds_table_max = std::min<size_t>(lds_table_max, 160 * 1024);
  return lds_bytes <= (double)lds_table_max ? MODE_GROUP_LDS : MODE_GROUP_GLOBAL;
}

int scan_grid(const Context* ctx, int mode, size_t num_chunks) {
  const int per_cu = mode == MODE_GROUP_LDS ? 2 : 8;
  return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)num_chunks, (int64_t)ctx->num_cus * per_cu));
}

std::unique_ptr<ph_result> new_result(Context* ctx, const std::vector<ph_segment*>& segs) {
  PH_HIP_CHECK(hipSetDevice(ctx->device));
  auto res = std::make_unique<ph_result>();
  res->ctx = ctx;
  res->stats.num_segments_processed = (int32_t)segs.size();
  for (auto* s : segs) res->stats.num_total_docs += s->num_docs;
  return res;
}

void group_streams(const KeySpace& ks, const ph_segment* seg, const uint32_t** gfwd, int32_t* gbits, const int32_t** gremap,
                   Scratch& scratch, std::vector<std::vector<int32_t>>& remap_keep, hipStream_t st) {
  for (size_t g = 0; g < ks.group_cols.size(); ++g) {
    const Column& c = *seg->columns.at(ks.group_cols[g]);
    if (c.sketch_words || !c.d_fwd.ptr) fail(PH_ERR_UNSUPPORTED, "group-by column " + ks.group_cols[g] + " has no forward index");
    gfwd[g] = c.d_fwd.as<uint32_t>();
    gbits[g] = c.bits;
    // a merge walk: both dictionaries are sorted and the union holds every entry of the segment's
    const Dictionary& gd = ks.gdicts[g]->dict;
    std::vector<int32_t> map((size_t)c.cardinality);
    bool identity = c.cardinality == gd.size;
    int64_t j = 0;
    for (int32_t v = 0; v < c.cardinality; ++v) {
      while (j < gd.size && gd.compare(j, c.dict, v) < 0) ++j;
      map[(size_t)v] = (int32_t)j;
      identity = identity && j == v;
    }
    if (identity) continue;
    int32_t* dm = scratch.alloc<int32_t>(map.size());
    remap_keep.push_back(std::move(map));
    PH_HIP_CHECK(hipMemcpyAsync(dm, remap_keep.back().data(), 4 * remap_keep.back().size(), hipMemcpyHostToDevice, st));
    gremap[g] = dm;
  }
}

void append_chunks(std::vector<Chunk>& chunks, int32_t seg_index, int32_t num_docs) {
  const int32_t nw = (int32_t)(((int64_t)num_docs + 63) / 64);
  for (int32_t w = 0; w < nw; w += kChunkWords)
    chunks.push_back(Chunk{seg_index, w, std::min<int32_t>(nw, w + kChunkWords), 0});
}

void add_scan_stats(ph_exec_stats& stats, const unsigned long long* seg_count, size_t num_device_segs, int64_t projected,
                    const std::vector<WhereBitmap>& bitmaps) {
  for (size_t d = 0; d < num_device_segs; ++d) {
    const int64_t docs = (int64_t)seg_count[d];
    stats.num_segments_matched += docs > 0;
    stats.num_docs_scanned += docs;
    stats.num_entries_scanned_post_filter += docs * projected;
  }
  for (auto& b : bitmaps) stats.num_entries_scanned_in_filter += b.entries;
}

void emit_keys(ph_result* res, const KeySpace& ks, const std::vector<int64_t>& rows) {
  const size_t R = rows.size();
  res->keys.resize(ks.group_cols.size());
  for (size_t c = 0; c < ks.group_cols.size(); ++c) {
    const Dictionary& d = ks.gdicts[c]->dict;
    const int32_t es = entry_size_of(d);
    res->key_types.push_back(d.type);
    res->key_entry_size.push_back(es);
    res->keys[c].assign(R * (size_t)es, 0);
    for (size_t r = 0; r < R; ++r)
      put_key(d, (rows[r] / ks.stride[c]) % ks.size(c), res->keys[c].data() + r * (size_t)es, es);
  }
}

void emit_rows(ph_result* res, const ph_query* q, const KeySpace& ks, const unsigned long long* n_host,
               const std::vector<int>& agg_slot, const uint8_t* tuples, size_t tuple_bytes) {
  int ns = 0;
  for (int s : agg_slot) ns = std::max(ns, s + 1);
  emit_rows(res, q, ks, n_host, agg_slot, tuples, std::vector<size_t>((size_t)ns, tuple_bytes));
}

void emit_rows(ph_result* res, const ph_query* q, const KeySpace& ks, const unsigned long long* n_host,
               const std::vector<int>& agg_slot, const uint8_t* tuples, const std::vector<size_t>& slot_bytes) {
  const int nagg = q->num_aggregations;
  std::vector<size_t> slot_base(slot_bytes.size(), 0);  // where slot v's [G] tuples start
  for (size_t v = 1; v < slot_bytes.size(); ++v) slot_base[v] = slot_base[v - 1] + (size_t)ks.G * slot_bytes[v - 1];
  res->agg_types.resize((size_t)nagg);
  res->agg_log2m.assign((size_t)nagg, 0);
  for (int k = 0; k < nagg; ++k) res->agg_types[(size_t)k] = q->aggregations[k].type;
  std::vector<int64_t> rows;
  if (ks.group_cols.empty()) rows.push_back(0);
  else
    for (int64_t g = 0; g < ks.G; ++g)
      if (n_host[g]) rows.push_back(g);
  const size_t R = rows.size();
  emit_keys(res, ks, rows);
  res->aggs.resize((size_t)nagg);
  for (int k = 0; k < nagg; ++k) {
    const bool count = q->aggregations[k].type == PH_AGG_COUNT;
    const size_t slot = count ? 0 : (size_t)agg_slot[(size_t)k];
    const size_t width = count ? 8 : slot_bytes[slot];
    res->aggs[(size_t)k].assign(width * R, 0);
    for (size_t r = 0; r < R; ++r) {
      const void* src = count ? reinterpret_cast<const uint8_t*>(n_host + rows[r])
                              : tuples + slot_base[slot] + width * (size_t)rows[r];
      memcpy(res->aggs[(size_t)k].data() + width * r, src, width);
    }
  }
  res->num_groups = (int64_t)R;
}

void finish_result(ph_result* res, int mode, double dev_ms, std::chrono::steady_clock::time_point t0) {
  const int plan_mode = mode == MODE_AGG ? 1 : (mode == MODE_GROUP_LDS ? 2 : 3);
  res->mode = plan_mode;
  res->stats.plan_mode = plan_mode;
  res->stats.num_devices = 1;
  res->stats.device_ms = dev_ms;
  res->stats.host_ms =
      std::max(0.0, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - dev_ms);
}

}  // namespace ph
