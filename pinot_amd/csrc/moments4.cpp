// moments4.cpp -- host-side plan of SKEWNESS / KURTOSIS (the reference's FourthMomentAggregationFunction over
// PinotFourthMoment), alone or beside COUNT(*), with or without a WHERE clause and a GROUP BY.
//
// The reference keeps a PinotFourthMoment (n, m1, m2, m3, m4) per result holder and folds every doc in with
// commons-math's one-pass update.  Here every argument column (a slot) gets a shift K for the call, taken from the first
// and last dictionary entries of the column in every queried segment, and the scan (scan_moments4.hip) accumulates n
// and the power sums S1..S4 of d = value - K:
//   * a column stored as INT or LONG whose range r = hi - lo over the call is below 2^32, in a call of at most 2^32
//     docs: K = lo, so 0 <= d <= r, and every power is split into 32-bit limbs with a 64-bit cell each -- M4_L8 when
//     r < 2^8 (4 cells), M4_L16 when r < 2^16 (6 cells), M4_L32 otherwise (10 cells);
//   * FLOAT / DOUBLE columns and integer columns past those bounds: M4_REAL, K the midpoint as a double and the four
//     sums in double.
// d comes from a per-segment table d_of[dictId] in per-call scratch, so the scan does one lookup per doc.
// k_moments4_finish then writes the tuple of every (group, slot); the two functions over one column share the slot and
// return the same tuple.
//
// Stage 1, the key space, the mode rule and the statistics are the variance plan's (moments.cpp), with this plan's
// bytes per key.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>

#include "ph_internal.h"

namespace ph {

namespace {

bool is_moment4(int32_t t) { return t == PH_AGG_SKEWNESS || t == PH_AGG_KURTOSIS; }

struct Slot {
  std::string col;
  int layout = M4_L8;
  int64_t shift = 0;  // K: an int64, or a double's bits (M4_REAL)
  bool is_int = true;
};

// the shift and the layout of one slot, from the column's range over the call's segments and the call's docs
void plan_slot(Slot& s, const std::vector<ph_segment*>& segs, double docs_queried) {
  int col_int = -1;
  bool any = false;
  int64_t ilo = 0, ihi = 0;
  double rlo = 0.0, rhi = 0.0;
  for (auto* seg : segs) {
    auto it = seg->columns.find(s.col);
    if (it == seg->columns.end()) fail(PH_ERR_BAD_QUERY, "Column not found: " + s.col + " in segment " + seg->name);
    const Column& c = *it->second;
    if (c.data_type == PH_STRING) fail(PH_ERR_UNSUPPORTED, "fourth-moment function on STRING column " + s.col);
    if (c.sketch_words) fail(PH_ERR_UNSUPPORTED, "fourth-moment function on sketch column " + s.col);
    const int ci = c.data_type == PH_INT || c.data_type == PH_LONG;
    if (col_int < 0) col_int = ci;
    else if (col_int != ci) fail(PH_ERR_UNSUPPORTED, "fourth-moment column with mixed integer/real types across segments");
    if (c.cardinality <= 0) continue;
    if (ci) {
      ilo = any ? std::min(ilo, c.dict.ints.front()) : c.dict.ints.front();
      ihi = any ? std::max(ihi, c.dict.ints.back()) : c.dict.ints.back();
    } else {
      rlo = any ? std::min(rlo, c.dict.reals.front()) : c.dict.reals.front();
      rhi = any ? std::max(rhi, c.dict.reals.back()) : c.dict.reals.back();
    }
    any = true;
  }
  s.is_int = col_int != 0;
  double kd = 0.5 * rlo + 0.5 * rhi;
  if (s.is_int) {
    const uint64_t r = (uint64_t)ihi - (uint64_t)ilo;
    // a limb cell holds docs x (2^32 - 1) at most: exact to 2^32 docs
    if (r < (1ull << 32) && docs_queried <= 4294967296.0) {
      s.layout = r < (1ull << 8) ? M4_L8 : (r < (1ull << 16) ? M4_L16 : M4_L32);
      s.shift = ilo;
      return;
    }
    kd = 0.5 * (double)ilo + 0.5 * (double)ihi;
  }
  s.layout = M4_REAL;
  memcpy(&s.shift, &kd, 8);
}

}  // namespace

bool has_moment4_aggregation(const ph_query* q) {
  if (!q || !q->aggregations) return false;
  for (int k = 0; k < q->num_aggregations; ++k)
    if (is_moment4(q->aggregations[k].type)) return true;
  return false;
}

void moments4_validate(const ph_query* q) {
  if (!q) fail(PH_ERR_INVALID_ARGUMENT, "null query");
  if (q->num_aggregations < 0 || (q->num_aggregations > 0 && !q->aggregations))
    fail(PH_ERR_INVALID_ARGUMENT, "bad aggregation list");
  std::vector<std::string> cols;
  for (int k = 0; k < q->num_aggregations; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.type >= PH_AGG_SUM && a.type <= PH_AGG_PERCENTILE) {
      static const char* fn[] = {"SUM", "MIN", "MAX", "DISTINCTCOUNTHLL", "DISTINCTCOUNT", "PERCENTILE"};
      fail(PH_ERR_UNSUPPORTED, std::string(fn[a.type - PH_AGG_SUM]) + " beside a fourth-moment function");
    }
    if (a.type >= PH_AGG_VARPOP && a.type <= PH_AGG_STDDEVSAMP)
      fail(PH_ERR_UNSUPPORTED, "variance function beside a fourth-moment function");
    if (a.type == PH_AGG_COVARPOP || a.type == PH_AGG_COVARSAMP)
      fail(PH_ERR_UNSUPPORTED, "covariance function beside a fourth-moment function");
    if (a.type != PH_AGG_COUNT && !is_moment4(a.type)) fail(PH_ERR_UNSUPPORTED, "aggregation type");
    if (a.filter) fail(PH_ERR_UNSUPPORTED, "a FILTER clause on or beside a fourth-moment function");
    if (a.type == PH_AGG_COUNT) continue;
    if (a.expr_op != PH_EXPR_NONE) fail(PH_ERR_UNSUPPORTED, "fourth-moment function of a 2-operand expression");
    if (!a.column) fail(PH_ERR_BAD_QUERY, "aggregation needs a column");
    if (std::find(cols.begin(), cols.end(), std::string(a.column)) == cols.end()) cols.push_back(a.column);
  }
  if ((int)cols.size() > kMMaxSlots)
    fail(PH_ERR_UNSUPPORTED,
         "more than " + std::to_string(kMMaxSlots) + " distinct columns under fourth-moment functions");
  if (q->num_aggregations > kMaxAggs) fail(PH_ERR_UNSUPPORTED, "too many aggregations");
  if (q->num_group_by > kMaxGroupCols) fail(PH_ERR_UNSUPPORTED, "too many group-by columns");
  if (q->min_segment_group_trim_size > 0 && q->num_group_by > 0 && q->num_order_by > 0)
    fail(PH_ERR_UNSUPPORTED, "fourth-moment functions with segment group trim (minSegmentGroupTrimSize)");
}

ph_result* moments4_execute(Context* ctx, const ph_query* q, ph_segment* const* segs_in, int32_t nseg) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  moments4_validate(q);
  if (nseg < 0 || (nseg > 0 && !segs_in)) fail(PH_ERR_INVALID_ARGUMENT, "bad segment list");
  std::vector<ph_segment*> segs(segs_in, segs_in + nseg);
  for (auto* s : segs)
    if (!s || s->ctx != ctx) fail(PH_ERR_INVALID_ARGUMENT, "segment is null or pinned on another context");
  if (q->interrupt && *q->interrupt) fail(PH_ERR_CANCELLED, "query interrupted");
  if (q->end_time_ms > 0) {
    const int64_t now = std::chrono::duration_cast<std::chrono::milliseconds>(
                            std::chrono::system_clock::now().time_since_epoch()).count();
    if (now > q->end_time_ms) fail(PH_ERR_CANCELLED, "query timed out (end time passed)");
  }

  // ---- slots (one per argument column), columns, the call's docs
  const int nagg = q->num_aggregations;
  std::vector<Slot> slots;
  std::vector<int> agg_slot(nagg, -1);
  for (int k = 0; k < nagg; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.type == PH_AGG_COUNT) continue;
    size_t at = 0;
    while (at < slots.size() && slots[at].col != a.column) ++at;
    if (at == slots.size()) {
      slots.emplace_back();
      slots.back().col = a.column;
    }
    agg_slot[k] = (int)at;
  }
  const int ns = (int)slots.size();
  std::vector<std::string> group_cols;
  for (int g = 0; g < q->num_group_by; ++g) {
    if (!q->group_by || !q->group_by[g]) fail(PH_ERR_INVALID_ARGUMENT, "null group-by column");
    group_cols.push_back(q->group_by[g]);
  }
  double docs_queried = 0.0;
  for (auto* s : segs) {
    docs_queried += (double)s->num_docs;
    for (auto& c : group_cols)
      if (!s->columns.count(c)) fail(PH_ERR_BAD_QUERY, "Column not found: " + c + " in segment " + s->name);
    for (int i = 0; i < q->num_predicates; ++i) {
      if (!q->predicates[i].column) fail(PH_ERR_BAD_QUERY, "predicate without column");
      if (!s->columns.count(q->predicates[i].column))
        fail(PH_ERR_BAD_QUERY, std::string("Column not found: ") + q->predicates[i].column);
    }
  }
  // per key: n, then 8 bytes per cell of every slot's layout; slot v's cells start at cell_off[v]
  size_t acc_per_key = 1;
  std::vector<size_t> cell_off((size_t)ns, 0);
  for (int v = 0; v < ns; ++v) {
    plan_slot(slots[(size_t)v], segs, docs_queried);
    cell_off[(size_t)v] = acc_per_key;
    acc_per_key += (size_t)m4_cells(slots[(size_t)v].layout);
  }
  constexpr size_t kTupleCells = sizeof(M4Tuple) / 8;

  // ---- per segment: how the WHERE clause plans (FilterPlanNode.run's isResultEmpty / isResultMatchingAll)
  std::vector<int32_t> cls(nseg, FP_ALL);
  for (int i = 0; i < nseg; ++i) {
    if (q->filter_root >= 0) cls[i] = filter_plan_class(q, q->filter_root, segs[i]);
    else if (segs[i]->num_docs == 0) cls[i] = FP_EMPTY;
  }

  // ---- key space
  std::vector<std::shared_ptr<GlobalDict>> gdicts;
  int64_t G = 1;
  for (auto& g : group_cols) {
    if (segs.empty()) fail(PH_ERR_UNSUPPORTED, "fourth-moment group-by without segments");
    gdicts.push_back(union_dictionary(g, segs));
    const int64_t sz = std::max<int64_t>(1, gdicts.back()->dict.size);
    if (G > (int64_t(1) << 40) / sz)
      fail(PH_ERR_UNSUPPORTED, "fourth-moment functions over a group key space beyond the dense tables");
    G *= sz;
  }
  const int64_t group_limit = q->num_groups_limit > 0 ? q->num_groups_limit : 100000;
  if (!group_cols.empty())
    for (int i = 0; i < nseg; ++i) {
      if (cls[i] == FP_EMPTY) continue;
      int64_t pp = 1;
      for (auto& g : group_cols) {
        const int64_t c = std::max<int64_t>(1, segs[i]->columns.at(g)->cardinality);
        pp = pp > (int64_t(1) << 40) / c ? int64_t(1) << 40 : pp * c;
      }
      // past the limit the groups the reference keeps depend on the order it meets them in
      if (std::min<int64_t>(pp, segs[i]->num_docs) >= group_limit)
        fail(PH_ERR_UNSUPPORTED, "fourth-moment functions where a segment could reach numGroupsLimit");
    }
  // n, the slots' cells and the 40-byte tuple per slot
  if ((double)G * 8.0 * (double)(acc_per_key + kTupleCells * (size_t)ns) > kDenseTableBudget)
    fail(PH_ERR_UNSUPPORTED, "fourth-moment functions over a group key space beyond the dense tables");
  int mode = MODE_AGG;
  if (!group_cols.empty()) {
    size_t lds_table_max = 64 * 1024;
    if (ctx->has(OPT_LDS_TABLE_MAX)) lds_table_max = (size_t)std::max<int64_t>(0, ctx->opt(OPT_LDS_TABLE_MAX));
    lds_table_max = std::min<size_t>(lds_table_max, 160 * 1024);
    mode = (double)G * 8.0 * (double)acc_per_key <= (double)lds_table_max ? MODE_GROUP_LDS : MODE_GROUP_GLOBAL;
  }

  PH_HIP_CHECK(hipSetDevice(ctx->device));
  auto res = std::make_unique<ph_result>();
  res->ctx = ctx;
  ph_exec_stats& stats = res->stats;
  stats.num_segments_processed = nseg;
  for (auto* s : segs) stats.num_total_docs += s->num_docs;
  double dev_ms = 0.0;

  LaneGuard lane(ctx);
  const hipStream_t st = lane.stream();
  // host sources of the stream's H2D copies: declared before `scratch`, whose destructor drains the stream, so they
  // outlive every copy also when the call unwinds by a throw
  std::vector<MSegment> msegs;
  std::vector<Chunk> chunks;
  std::vector<std::vector<int32_t>> remap_keep;
  std::vector<std::vector<int64_t>> d_of_keep;
  std::vector<unsigned long long> host_tables;  // (and the target of the result's D2H copies)
  Scratch scratch(ctx, st);

  // ---- stage 1: the WHERE clause's doc bitmap per segment where it neither matches all nor is empty
  std::vector<const unsigned long long*> bitmap(nseg, nullptr);
  std::vector<int64_t> bm_entries(nseg, 0);
  for (int i = 0; i < nseg; ++i) {
    if (cls[i] == FP_EMPTY || cls[i] == FP_ALL) continue;
    const int64_t need = std::max<int64_t>(1, ((int64_t)segs[i]->num_docs + 63) / 64);
    unsigned long long* words = scratch.alloc<unsigned long long>((size_t)need);
    ph_query qc = *q;
    ph_aggregation cnt{};
    cnt.type = PH_AGG_COUNT;
    qc.num_group_by = 0;
    qc.group_by = nullptr;
    qc.num_aggregations = 1;
    qc.aggregations = &cnt;
    qc.num_order_by = 0;
    qc.order_by = nullptr;
    qc.min_segment_group_trim_size = -1;
    qc.skip_star_tree = 1;
    const int64_t off[1] = {0};
    FilterDocset fd{words, off, need};
    DenseArgs d{0, nullptr, 0, 0, nullptr};
    d.docset = &fd;
    ph_segment* one[1] = {segs[i]};
    std::unique_ptr<ph_result> r(query_execute_impl(ctx, &qc, one, 1, &d));  // drains its stream before it returns
    bitmap[i] = words;
    bm_entries[i] = r->stats.num_entries_scanned_in_filter;
    dev_ms += r->stats.device_ms;
  }
  if (q->interrupt && *q->interrupt) fail(PH_ERR_CANCELLED, "query interrupted");

  // ---- stage 2: device segments (with each slot's d_of table), chunks, tables
  for (int i = 0; i < nseg; ++i) {
    if (cls[i] == FP_EMPTY || segs[i]->num_docs == 0) continue;
    MSegment d{};
    d.num_docs = segs[i]->num_docs;
    d.mask = bitmap[i];
    for (size_t g = 0; g < group_cols.size(); ++g) {
      const Column& c = *segs[i]->columns.at(group_cols[g]);
      if (c.sketch_words || !c.d_fwd.ptr) fail(PH_ERR_UNSUPPORTED, "group-by column " + group_cols[g] + " has no forward index");
      d.gfwd[g] = c.d_fwd.as<uint32_t>();
      d.gbits[g] = c.bits;
      const Dictionary& gd = gdicts[g]->dict;
      std::vector<int32_t> map((size_t)c.cardinality);
      bool identity = c.cardinality == gd.size;
      int64_t j = 0;
      for (int32_t v = 0; v < c.cardinality; ++v) {
        while (j < gd.size && gd.compare(j, c.dict, v) < 0) ++j;
        map[(size_t)v] = (int32_t)j;
        identity = identity && j == v;
      }
      if (!identity) {
        int32_t* dm = scratch.alloc<int32_t>(map.size());
        remap_keep.push_back(std::move(map));
        PH_HIP_CHECK(hipMemcpyAsync(dm, remap_keep.back().data(), 4 * remap_keep.back().size(), hipMemcpyHostToDevice, st));
        d.gremap[g] = dm;
      }
    }
    for (int v = 0; v < ns; ++v) {
      const Slot& s = slots[(size_t)v];
      const Column& c = *segs[i]->columns.at(s.col);
      if (!c.d_fwd.ptr) fail(PH_ERR_UNSUPPORTED, "fourth-moment column " + s.col + " has no forward index");
      std::vector<int64_t> tab((size_t)std::max(1, c.cardinality), 0);
      double kd;
      memcpy(&kd, &s.shift, 8);
      for (int32_t id = 0; id < c.cardinality; ++id) {
        if (s.layout != M4_REAL) {
          tab[(size_t)id] = (int64_t)((uint64_t)c.dict.ints[(size_t)id] - (uint64_t)s.shift);  // 0 <= d < 2^32
        } else {
          const double x = (s.is_int ? (double)c.dict.ints[(size_t)id] : c.dict.reals[(size_t)id]) - kd;
          memcpy(&tab[(size_t)id], &x, 8);
        }
      }
      long long* dt = scratch.alloc<long long>(tab.size());
      d_of_keep.push_back(std::move(tab));
      PH_HIP_CHECK(hipMemcpyAsync(dt, d_of_keep.back().data(), 8 * d_of_keep.back().size(), hipMemcpyHostToDevice, st));
      d.vfwd[v] = c.d_fwd.as<uint32_t>();
      d.d_of[v] = dt;
      d.vbits[v] = c.bits;
    }
    const int32_t nw = (int32_t)(((int64_t)d.num_docs + 63) / 64);
    for (int32_t w = 0; w < nw; w += kChunkWords)
      chunks.push_back(Chunk{(int32_t)msegs.size(), w, std::min<int32_t>(nw, w + kChunkWords), 0});
    msegs.push_back(d);
  }
  // u64 cells: [segments] matched docs | n[G] | per slot its layout's cells, [G] each | per slot the M4Tuple[G] of the
  // finish
  const size_t nms = msegs.size();
  const size_t cnt_cells = std::max<size_t>(1, nms);
  const size_t out_off = cnt_cells + (size_t)G * acc_per_key;
  const size_t cells = out_off + kTupleCells * (size_t)G * (size_t)ns;
  host_tables.assign(cells, 0ull);
  {  // no launch (no segment left to scan): every tuple is the empty one, (0, NaN, NaN, NaN, NaN)
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const M4Tuple empty{0, nan, nan, nan, nan};
    for (size_t i = 0; i < (size_t)G * (size_t)ns; ++i) memcpy(&host_tables[out_off + kTupleCells * i], &empty, sizeof(empty));
  }
  if (!chunks.empty()) {
    unsigned long long* tables = scratch.alloc<unsigned long long>(cells);
    MSegment* d_segs = scratch.alloc<MSegment>(nms);
    Chunk* d_chunks = scratch.alloc<Chunk>(chunks.size());
    PH_HIP_CHECK(hipMemcpyAsync(d_segs, msegs.data(), sizeof(MSegment) * nms, hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), sizeof(Chunk) * chunks.size(), hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_start, st));
    PH_HIP_CHECK(hipMemsetAsync(tables, 0, 8 * out_off, st));
    unsigned long long* n_tab = tables + cnt_cells;
    M4FinishParams fin{};
    fin.num_groups = G;
    fin.num_slots = ns;
    fin.n = n_tab;
    for (int v = 0; v < ns; ++v) {
      fin.layout[v] = slots[(size_t)v].layout;
      fin.shift[v] = slots[(size_t)v].shift;
      fin.cells[v] = n_tab + (size_t)G * cell_off[(size_t)v];
      fin.out[v] = reinterpret_cast<M4Tuple*>(tables + out_off + kTupleCells * (size_t)G * (size_t)v);
    }
    const int per_cu = mode == MODE_GROUP_LDS ? 2 : 8;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)chunks.size(), (int64_t)ctx->num_cus * per_cu));
    // one launch per layout among the slots; the first one counts the docs (n and the segments' matched docs)
    bool counted = false;
    for (int layout = M4_L8; layout <= M4_REAL; ++layout) {
      M4Params mp{};
      mp.segs = d_segs;
      mp.chunks = d_chunks;
      mp.chunk_end = (int32_t)chunks.size();
      mp.num_group_cols = (int32_t)group_cols.size();
      int64_t stride = 1;
      for (int g = (int)group_cols.size() - 1; g >= 0; --g) {
        mp.group_stride[g] = stride;
        stride *= std::max<int64_t>(1, gdicts[(size_t)g]->dict.size);
      }
      mp.num_groups = G;
      for (int v = 0; v < ns; ++v) {
        if (slots[(size_t)v].layout != layout) continue;
        const int at = mp.num_slots++;
        mp.slot_col[at] = v;
        mp.cells[at] = n_tab + (size_t)G * cell_off[(size_t)v];
      }
      if (!mp.num_slots) continue;
      if (!counted) {
        mp.n = n_tab;
        mp.seg_count = tables;
        counted = true;
      }
      launch_scan_moments4(mp, mode, layout, grid, st);
    }
    launch_moments4_finish(fin, st);
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_stop, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data(), tables, 8 * (cnt_cells + (size_t)G), hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data() + out_off, tables + out_off, 8 * (cells - out_off),
                                hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0.f;
    PH_HIP_CHECK(hipEventElapsedTime(&ms, lane.lane->ev_start, lane.lane->ev_stop));
    dev_ms += (double)ms;
  }
  stats.scan_kernel = PH_KERNEL_SCAN_MOMENTS4;
  const unsigned long long* seg_count = host_tables.data();
  const unsigned long long* n_host = host_tables.data() + cnt_cells;
  auto tuple_of = [&](int slot, int64_t g) {
    return reinterpret_cast<const uint8_t*>(host_tables.data() + out_off + kTupleCells * ((size_t)G * (size_t)slot + (size_t)g));
  };

  // ---- statistics: matched docs, the WHERE clause's ordinary statistic, docs x projected columns
  const int64_t projected = (int64_t)group_cols.size() + ns;
  for (size_t d = 0; d < nms; ++d) {
    const int64_t docs = (int64_t)seg_count[d];
    stats.num_segments_matched += docs > 0;
    stats.num_docs_scanned += docs;
    stats.num_entries_scanned_post_filter += docs * projected;
  }
  for (int i = 0; i < nseg; ++i) stats.num_entries_scanned_in_filter += bm_entries[i];

  // ---- result rows: a group is a row when it holds a doc; an aggregation-only query has one row, the empty tuple
  // where nothing matched
  res->agg_types.resize((size_t)nagg);
  res->agg_log2m.assign((size_t)nagg, 0);
  for (int k = 0; k < nagg; ++k) res->agg_types[(size_t)k] = q->aggregations[k].type;
  std::vector<int64_t> rows;
  if (group_cols.empty()) rows.push_back(0);
  else
    for (int64_t g = 0; g < G; ++g)
      if (n_host[g]) rows.push_back(g);
  const size_t R = rows.size();
  int64_t stride = 1;
  std::vector<int64_t> key_stride(group_cols.size(), 1);
  for (int g = (int)group_cols.size() - 1; g >= 0; --g) {
    key_stride[(size_t)g] = stride;
    stride *= std::max<int64_t>(1, gdicts[(size_t)g]->dict.size);
  }
  res->keys.resize(group_cols.size());
  for (size_t c = 0; c < group_cols.size(); ++c) {
    const Dictionary& d = gdicts[c]->dict;
    const int32_t es = entry_size_of(d);
    res->key_types.push_back(d.type);
    res->key_entry_size.push_back(es);
    res->keys[c].assign(R * (size_t)es, 0);
    const int64_t sz = std::max<int64_t>(1, d.size);
    for (size_t r = 0; r < R; ++r) put_key(d, (rows[r] / key_stride[c]) % sz, res->keys[c].data() + r * (size_t)es, es);
  }
  res->aggs.resize((size_t)nagg);
  for (int k = 0; k < nagg; ++k) {
    const bool count = q->aggregations[k].type == PH_AGG_COUNT;
    const size_t width = count ? 8 : sizeof(M4Tuple);
    res->aggs[(size_t)k].assign(width * R, 0);
    for (size_t r = 0; r < R; ++r) {
      const void* src = count ? reinterpret_cast<const uint8_t*>(n_host + rows[r]) : tuple_of(agg_slot[k], rows[r]);
      memcpy(res->aggs[(size_t)k].data() + width * r, src, width);
    }
  }
  res->num_groups = (int64_t)R;
  const int plan_mode = mode == MODE_AGG ? 1 : (mode == MODE_GROUP_LDS ? 2 : 3);
  res->mode = plan_mode;
  stats.plan_mode = plan_mode;
  stats.num_devices = 1;
  stats.device_ms = dev_ms;
  stats.host_ms = std::max(0.0, std::chrono::duration<double, std::milli>(clock::now() - t0).count() - dev_ms);
  return res.release();
}

}  // namespace ph
