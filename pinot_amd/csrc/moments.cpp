// moments.cpp -- host-side plan of the variance family: VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP (the reference's
// VarianceAggregationFunction), alone or beside COUNT(*), with or without a WHERE clause and a GROUP BY.
//
// The reference keeps a VarianceTuple (count, sum, m2) per result holder and folds every doc in with Chan's update
// (VarianceAggregationFunction.java:80-121, VarianceTuple.apply :35-44).  Here every argument column (a slot) gets a
// shift K for the call, taken from the first and last dictionary entries of the column in every queried segment, and
// the scan (scan_moments.hip) accumulates n, sum(d) and sum(d^2) of d = value - K:
//   * a column stored as INT or LONG: K = lo + (hi - lo) / 2 and dmax = max(hi - K, K - lo); with N the docs of the
//     call's segments the integer form holds when dmax N < 2^63 and dmax^2 N < 2^127 (every INT column; a LONG column
//     whose range is below about 2^47 at 2^32 docs) -- narrow when dmax^2 N < 2^64 (sum(d^2) is one u64 cell that
//     never carries), wide otherwise (a (lo, hi) pair of cells);
//   * FLOAT / DOUBLE columns and integer columns past those bounds: the real form, K the midpoint as a double and the
//     two sums in double.
// d comes from a per-segment table d_of[dictId] in per-call scratch, so the scan does one lookup per doc.
// k_moments_finish then writes the tuple of every (group, slot); the four functions over one column share the slot and
// return the same tuple.
//
// Stage 1 is the filtered plan's (filtered.cpp): a WHERE clause that neither matches all nor is empty on a segment runs
// through query_execute_impl's COUNT(*) + doc bitmap form and leaves the bitmap, its matched docs and its ordinary
// numEntriesScannedInFilter.  Group keys are the call's union-dictionary ids over one dense key space.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "ph_internal.h"

namespace ph {

namespace {

bool is_moment(int32_t t) { return t >= PH_AGG_VARPOP && t <= PH_AGG_STDDEVSAMP; }

struct Slot {
  std::string col;
  int form = MFORM_NARROW;
  int64_t shift = 0;  // K: an int64, or a double's bits (MFORM_REAL)
  bool is_int = true;
};

// the shift and the form of one slot, from the column's range over the call's segments and the call's docs
void plan_slot(Slot& s, const std::vector<ph_segment*>& segs, double docs_queried) {
  int col_int = -1;
  bool any = false;
  int64_t ilo = 0, ihi = 0;
  double rlo = 0.0, rhi = 0.0;
  for (auto* seg : segs) {
    auto it = seg->columns.find(s.col);
    if (it == seg->columns.end()) fail(PH_ERR_BAD_QUERY, "Column not found: " + s.col + " in segment " + seg->name);
    const Column& c = *it->second;
    if (c.data_type == PH_STRING) fail(PH_ERR_UNSUPPORTED, "variance function on STRING column " + s.col);
    if (c.sketch_words) fail(PH_ERR_UNSUPPORTED, "variance function on sketch column " + s.col);
    const int ci = c.data_type == PH_INT || c.data_type == PH_LONG;
    if (col_int < 0) col_int = ci;
    else if (col_int != ci) fail(PH_ERR_UNSUPPORTED, "variance column with mixed integer/real types across segments");
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
    const uint64_t half = ((uint64_t)ihi - (uint64_t)ilo) / 2;
    const int64_t K = (int64_t)((uint64_t)ilo + half);
    const uint64_t dmax = std::max((uint64_t)ihi - (uint64_t)K, (uint64_t)K - (uint64_t)ilo);
    const unsigned __int128 N = (uint64_t)std::max(1.0, docs_queried);
    const unsigned __int128 one = 1;
    const bool sum_fits = dmax < (one << 63) && (unsigned __int128)dmax * N < (one << 63);
    if (sum_fits) {  // (dmax < 2^63 here, so its square fits 128 bits)
      const unsigned __int128 sq = (unsigned __int128)dmax * dmax;
      if (sq <= ((one << 127) - 1) / N) {
        s.form = sq <= ((one << 64) - 1) / N ? MFORM_NARROW : MFORM_WIDE;
        s.shift = K;
        return;
      }
    }
    kd = 0.5 * (double)ilo + 0.5 * (double)ihi;
  }
  s.form = MFORM_REAL;
  memcpy(&s.shift, &kd, 8);
}

}  // namespace

bool has_moment_aggregation(const ph_query* q) {
  if (!q || !q->aggregations) return false;
  for (int k = 0; k < q->num_aggregations; ++k)
    if (is_moment(q->aggregations[k].type)) return true;
  return false;
}

void moments_validate(const ph_query* q) {
  if (!q) fail(PH_ERR_INVALID_ARGUMENT, "null query");
  if (q->num_aggregations < 0 || (q->num_aggregations > 0 && !q->aggregations))
    fail(PH_ERR_INVALID_ARGUMENT, "bad aggregation list");
  std::vector<std::string> cols;
  for (int k = 0; k < q->num_aggregations; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.type >= PH_AGG_SUM && a.type <= PH_AGG_PERCENTILE) {
      static const char* fn[] = {"SUM", "MIN", "MAX", "DISTINCTCOUNTHLL", "DISTINCTCOUNT", "PERCENTILE"};
      fail(PH_ERR_UNSUPPORTED, std::string(fn[a.type - PH_AGG_SUM]) + " beside a variance function");
    }
    if (a.type != PH_AGG_COUNT && !is_moment(a.type)) fail(PH_ERR_UNSUPPORTED, "aggregation type");
    if (a.filter) fail(PH_ERR_UNSUPPORTED, "a FILTER clause on or beside a variance function");
    if (a.type == PH_AGG_COUNT) continue;
    if (a.expr_op != PH_EXPR_NONE) fail(PH_ERR_UNSUPPORTED, "variance function of a 2-operand expression");
    if (!a.column) fail(PH_ERR_BAD_QUERY, "aggregation needs a column");
    if (std::find(cols.begin(), cols.end(), std::string(a.column)) == cols.end()) cols.push_back(a.column);
  }
  if ((int)cols.size() > kMMaxSlots)
    fail(PH_ERR_UNSUPPORTED, "more than " + std::to_string(kMMaxSlots) + " distinct columns under variance functions");
  if (q->num_aggregations > kMaxAggs) fail(PH_ERR_UNSUPPORTED, "too many aggregations");
  if (q->num_group_by > kMaxGroupCols) fail(PH_ERR_UNSUPPORTED, "too many group-by columns");
  if (q->min_segment_group_trim_size > 0 && q->num_group_by > 0 && q->num_order_by > 0)
    fail(PH_ERR_UNSUPPORTED, "variance functions with segment group trim (minSegmentGroupTrimSize)");
}

ph_result* moments_execute(Context* ctx, const ph_query* q, ph_segment* const* segs_in, int32_t nseg) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  moments_validate(q);
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
  int cell_bytes = 8;  // per key: n, then 16 bytes per narrow or real slot, 24 per wide one
  for (auto& s : slots) {
    plan_slot(s, segs, docs_queried);
    cell_bytes += s.form == MFORM_WIDE ? 24 : 16;
  }

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
    if (segs.empty()) fail(PH_ERR_UNSUPPORTED, "variance group-by without segments");
    gdicts.push_back(union_dictionary(g, segs));
    const int64_t sz = std::max<int64_t>(1, gdicts.back()->dict.size);
    if (G > (int64_t(1) << 40) / sz) fail(PH_ERR_UNSUPPORTED, "variance functions over a group key space beyond the dense tables");
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
        fail(PH_ERR_UNSUPPORTED, "variance functions where a segment could reach numGroupsLimit");
    }
  // n, three accumulator cells and the 24-byte tuple per slot
  if ((double)G * (8.0 + 48.0 * ns) > kDenseTableBudget)
    fail(PH_ERR_UNSUPPORTED, "variance functions over a group key space beyond the dense tables");
  int mode = MODE_AGG;
  if (!group_cols.empty()) {
    size_t lds_table_max = 64 * 1024;
    if (ctx->has(OPT_LDS_TABLE_MAX)) lds_table_max = (size_t)std::max<int64_t>(0, ctx->opt(OPT_LDS_TABLE_MAX));
    lds_table_max = std::min<size_t>(lds_table_max, 160 * 1024);
    mode = (double)G * cell_bytes <= (double)lds_table_max ? MODE_GROUP_LDS : MODE_GROUP_GLOBAL;
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
  std::vector<int> mseg_src;
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
      if (!c.d_fwd.ptr) fail(PH_ERR_UNSUPPORTED, "variance column " + s.col + " has no forward index");
      std::vector<int64_t> tab((size_t)std::max(1, c.cardinality), 0);
      double kd;
      memcpy(&kd, &s.shift, 8);
      for (int32_t id = 0; id < c.cardinality; ++id) {
        if (s.form != MFORM_REAL) {
          tab[(size_t)id] = (int64_t)((uint64_t)c.dict.ints[(size_t)id] - (uint64_t)s.shift);
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
    mseg_src.push_back(i);
    msegs.push_back(d);
  }
  // u64 cells: [segments] matched docs | n[G] | per slot S1[G], S2lo[G], S2hi[G] | per slot the MTuple[G] of the finish
  const size_t nms = msegs.size();
  const size_t cnt_cells = std::max<size_t>(1, nms);
  const size_t acc_cells = (size_t)G * (1 + 3 * (size_t)ns);
  const size_t out_off = cnt_cells + acc_cells;
  const size_t cells = out_off + 3 * (size_t)G * (size_t)ns;
  host_tables.assign(cells, 0ull);  // (an MTuple of zero bits is (0, 0.0, 0.0))
  if (!chunks.empty()) {
    unsigned long long* tables = scratch.alloc<unsigned long long>(cells);
    MSegment* d_segs = scratch.alloc<MSegment>(nms);
    Chunk* d_chunks = scratch.alloc<Chunk>(chunks.size());
    PH_HIP_CHECK(hipMemcpyAsync(d_segs, msegs.data(), sizeof(MSegment) * nms, hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), sizeof(Chunk) * chunks.size(), hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_start, st));
    PH_HIP_CHECK(hipMemsetAsync(tables, 0, 8 * out_off, st));
    unsigned long long* n_tab = tables + cnt_cells;
    auto cell = [&](int slot, int which) { return n_tab + (size_t)G * (1 + 3 * (size_t)slot + (size_t)which); };
    MFinishParams fin{};
    fin.num_groups = G;
    fin.num_slots = ns;
    fin.n = n_tab;
    for (int v = 0; v < ns; ++v) {
      fin.form[v] = slots[(size_t)v].form;
      fin.shift[v] = slots[(size_t)v].shift;
      fin.s1[v] = cell(v, 0);
      fin.s2lo[v] = cell(v, 1);
      fin.s2hi[v] = cell(v, 2);
      fin.out[v] = reinterpret_cast<MTuple*>(tables + out_off + 3 * (size_t)G * (size_t)v);
    }
    const int per_cu = mode == MODE_GROUP_LDS ? 2 : 8;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)chunks.size(), (int64_t)ctx->num_cus * per_cu));
    // one launch per form among the slots; the first one counts the docs (n and the segments' matched docs)
    bool counted = false;
    for (int form = MFORM_NARROW; form <= MFORM_REAL; ++form) {
      MParams mp{};
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
        if (slots[(size_t)v].form != form) continue;
        const int at = mp.num_slots++;
        mp.slot_col[at] = v;
        mp.s1[at] = cell(v, 0);
        mp.s2lo[at] = cell(v, 1);
        mp.s2hi[at] = cell(v, 2);
      }
      if (!mp.num_slots) continue;
      if (!counted) {
        mp.n = n_tab;
        mp.seg_count = tables;
        counted = true;
      }
      launch_scan_moments(mp, mode, form, grid, st);
    }
    launch_moments_finish(fin, st);
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_stop, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data(), tables, 8 * (cnt_cells + (size_t)G), hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data() + out_off, tables + out_off, 8 * (cells - out_off),
                                hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0.f;
    PH_HIP_CHECK(hipEventElapsedTime(&ms, lane.lane->ev_start, lane.lane->ev_stop));
    dev_ms += (double)ms;
  }
  stats.scan_kernel = PH_KERNEL_SCAN_MOMENTS;
  const unsigned long long* seg_count = host_tables.data();
  const unsigned long long* n_host = host_tables.data() + cnt_cells;
  auto tuple_of = [&](int slot, int64_t g) {
    return reinterpret_cast<const uint8_t*>(host_tables.data() + out_off + 3 * ((size_t)G * (size_t)slot + (size_t)g));
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

  // ---- result rows: a group is a row when it holds a doc; an aggregation-only query has one row, (0, 0.0, 0.0)
  // where nothing matched (VarianceAggregationFunction.extractAggregationResult :190-197)
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
    const size_t width = count ? 8 : sizeof(MTuple);
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
