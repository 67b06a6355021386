// withtime.cpp -- host-side plan of FIRSTWITHTIME / LASTWITHTIME(dataCol, timeCol, 'type') (the reference's
// FirstWithTimeAggregationFunction / LastWithTimeAggregationFunction and their First|Last{Int,Long,Float,Double}
// ValueWithTime subclasses, AggregationFunctionFactory.java:201-254), alone or beside COUNT(*), with or without a WHERE
// clause and a GROUP BY.
//
// The winning doc of a row depends on the time column and the direction only, so a slot is one distinct (time column,
// direction) pair and any number of aggregations over different data columns share its cell.  The time of a doc is
// timeValSet.getLongValuesSV() (LastIntValueWithTimeAggregationFunction.java:71): this plan casts every dictionary
// entry of a time column to long once, as Java's (long) does, ranks the distinct results over the call and gives the
// scan (scan_withtime.hip) a uint32 table hi_of[dictId] per (segment, slot): rank + 1 for LAST, T - rank for FIRST.
// The scan keeps the largest key per (row, slot); k_withtime_finish reads each aggregation's data column at the one
// doc its cell names.
//
// Stage 1, the key space, the mode rule, the statistics and the assembly of the result are the shared steps of
// scan_plan.h.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>

#include "scan_plan.h"

namespace ph {

namespace {

constexpr Family kFamily{"with-time", "with-time functions"};

struct Slot {
  std::string tcol;
  bool first = false;
  int tc = 0;  // index of tcol among the distinct time columns
};

struct WAgg {
  int k = 0;  // index in the query
  std::string dcol;
  int32_t declared = PH_INT;
  int slot = 0;
};

// (long) of a double as Java casts it: truncation toward zero, NaN is 0, the rest saturates
int64_t java_long(double x) {
  if (std::isnan(x)) return 0;
  if (x >= 9223372036854775807.0) return INT64_MAX;
  if (x <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)x;
}

int64_t time_of(const Column& c, int32_t id) {
  const bool is_int = c.data_type == PH_INT || c.data_type == PH_LONG;
  return is_int ? c.dict.ints[(size_t)id] : java_long(c.dict.reals[(size_t)id]);
}

const char* type_name(int32_t t) {
  static const char* names[] = {"INT", "LONG", "FLOAT", "DOUBLE", "STRING"};
  return t >= PH_INT && t <= PH_STRING ? names[t] : "?";
}

// DEFAULT_VALUE_TIME_PAIR of the subclass (Last|First{Int,Long,Float,Double}ValueWithTimeAggregationFunction.java:42-44):
// Integer.MIN_VALUE, Long.MIN_VALUE, Float.NaN, Double.NaN; time Long.MIN_VALUE for LAST and Long.MAX_VALUE for FIRST
void default_pair(int32_t declared, bool first, int64_t* value, int64_t* time) {
  const double nan = std::numeric_limits<double>::quiet_NaN();  // (double) Float.NaN is Double.NaN's bits too
  if (declared == PH_INT) *value = (int64_t)INT32_MIN;
  else if (declared == PH_LONG) *value = INT64_MIN;
  else memcpy(value, &nan, 8);
  *time = first ? INT64_MAX : INT64_MIN;
}

const ph_with_time_args& args_of(const ph_query* q, int k) {
  if (!q->with_time) fail(PH_ERR_BAD_QUERY, "FIRSTWITHTIME / LASTWITHTIME without its declared type (ph_query.with_time)");
  return q->with_time[k];
}

}  // namespace

bool has_with_time_aggregation(const ph_query* q) {
  if (!q || !q->aggregations) return false;
  for (int k = 0; k < q->num_aggregations; ++k)
    if (is_with_time(q->aggregations[k].type)) return true;
  return false;
}

void withtime_validate(const ph_query* q) {
  check_query(q);
  for (int k = 0; k < q->num_aggregations; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    refuse_plain_beside(kFamily, a);
    if (is_moment(a.type)) fail(PH_ERR_UNSUPPORTED, "variance function beside a with-time function");
    if (is_comoment(a.type)) fail(PH_ERR_UNSUPPORTED, "covariance function beside a with-time function");
    if (is_moment4(a.type)) fail(PH_ERR_UNSUPPORTED, "fourth-moment function beside a with-time function");
    if (a.type == PH_AGG_HISTOGRAM) fail(PH_ERR_UNSUPPORTED, "histogram function beside a with-time function");
    if (a.type != PH_AGG_COUNT && !is_with_time(a.type)) fail(PH_ERR_UNSUPPORTED, "aggregation type");
    if (a.filter) fail(PH_ERR_UNSUPPORTED, "a FILTER clause on or beside a with-time function");
    if (a.type == PH_AGG_COUNT) continue;
    if (a.expr_op != PH_EXPR_NONE) fail(PH_ERR_UNSUPPORTED, "with-time function of a 2-operand expression");
    if (!a.column || !a.column2) fail(PH_ERR_BAD_QUERY, "a with-time function needs a data column and a time column");
    const int32_t t = args_of(q, k).data_type;
    if (t == PH_STRING) fail(PH_ERR_UNSUPPORTED, "with-time function with declared type STRING");
    if (t < PH_INT || t > PH_DOUBLE) fail(PH_ERR_BAD_QUERY, "with-time function with an unknown declared type");
  }
  check_shape(kFamily, q);
}

ph_result* withtime_execute(Context* ctx, const ph_query* q, ph_segment* const* segs_in, int32_t nseg) {
  const auto t0 = std::chrono::steady_clock::now();
  withtime_validate(q);
  const std::vector<ph_segment*> segs = check_call(ctx, q, segs_in, nseg);

  // ---- slots (one per distinct (time column, direction) pair), the with-time aggregations, columns, the call's docs
  const int nagg = q->num_aggregations;
  std::vector<Slot> slots;
  std::vector<WAgg> waggs;
  std::vector<std::string> time_cols, proj_cols;  // distinct time columns; distinct data and time columns
  std::vector<int> agg_w(nagg, -1);
  bool counting = false;
  for (int k = 0; k < nagg; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.type == PH_AGG_COUNT) {
      counting = true;
      continue;
    }
    Slot s;
    s.tcol = a.column2;
    s.first = a.type == PH_AGG_FIRSTWITHTIME;
    size_t at = 0;
    while (at < slots.size() && !(slots[at].tcol == s.tcol && slots[at].first == s.first)) ++at;
    if (at == slots.size()) {
      s.tc = (int)(std::find(time_cols.begin(), time_cols.end(), s.tcol) - time_cols.begin());
      if (s.tc == (int)time_cols.size()) time_cols.push_back(s.tcol);
      slots.push_back(s);
    }
    agg_w[k] = (int)waggs.size();
    waggs.push_back(WAgg{k, a.column, q->with_time[k].data_type, (int)at});
    for (const char* c : {a.column, a.column2})
      if (std::find(proj_cols.begin(), proj_cols.end(), c) == proj_cols.end()) proj_cols.push_back(c);
  }
  const int ns = (int)slots.size(), nw = (int)waggs.size();
  if (ns > kWMaxSlots)
    fail(PH_ERR_UNSUPPORTED, "more than " + std::to_string(kWMaxSlots) + " distinct (time column, direction) pairs under with-time functions");
  const std::vector<std::string> group_cols = group_columns(q);
  check_columns(q, segs, group_cols);
  double docs_queried = 0.0;
  for (auto* s : segs) docs_queried += (double)s->num_docs;
  if (docs_queried >= 4294967295.0) fail(PH_ERR_UNSUPPORTED, "with-time functions over a call of 2^32 - 1 docs or more");
  for (auto& tc : time_cols) numeric_range(kFamily, tc, segs);  // refuses STRING, sketch and mixed-type time columns
  for (const WAgg& w : waggs)
    for (auto* seg : segs) {
      const Column& c = column_in(seg, w.dcol);
      if (c.data_type == PH_STRING) fail(PH_ERR_UNSUPPORTED, "with-time function on STRING column " + w.dcol);
      if (c.sketch_words) fail(PH_ERR_UNSUPPORTED, "with-time function on sketch column " + w.dcol);
      // the declared type reads the column through get{Int,Long,Float,Double}ValuesSV: exact for the stored type and
      // for INT -> LONG, INT -> DOUBLE and FLOAT -> DOUBLE only
      const bool exact = w.declared == c.data_type || (c.data_type == PH_INT && (w.declared == PH_LONG || w.declared == PH_DOUBLE)) ||
                         (c.data_type == PH_FLOAT && w.declared == PH_DOUBLE);
      if (!exact)
        fail(PH_ERR_UNSUPPORTED, std::string("with-time function declaring ") + type_name(w.declared) + " over " +
                                     type_name(c.data_type) + " column " + w.dcol + ": neither its stored type nor an exact widening of it");
    }

  // ---- the WHERE clause's class per segment, the key space, the mode
  std::vector<int32_t> cls((size_t)nseg);
  for (int i = 0; i < nseg; ++i) cls[i] = where_class(q, segs[i]);
  const KeySpace ks = key_space(kFamily, group_cols, segs);
  const int64_t G = ks.G;
  refuse_group_limit(kFamily, q, ks, segs, cls);
  // tables: the cells, n and the pairs; in LDS the cells and, when the query counts, n
  const int mode = choose_mode(ctx, kFamily, ks, (double)G * (8.0 * ns + 8.0 + 16.0 * nw),
                               (double)G * (8.0 * ns + (counting ? 8.0 : 0.0)));

  auto res = new_result(ctx, segs);
  ph_exec_stats& stats = res->stats;
  double dev_ms = 0.0;

  LaneGuard lane(ctx);
  const hipStream_t st = lane.stream();
  // host sources of the stream's H2D copies: declared before `scratch`, whose destructor drains the stream, so they
  // outlive every copy also when the call unwinds by a throw
  std::vector<WSegment> wsegs;
  std::vector<WFinSeg> fsegs;
  std::vector<WFinAgg> faggs((size_t)nw);
  std::vector<Chunk> chunks;
  std::vector<std::vector<int32_t>> remap_keep;
  std::vector<std::vector<uint32_t>> hi_keep;
  std::vector<std::vector<int64_t>> times((size_t)time_cols.size());  // time_of_rank per time column
  std::vector<unsigned long long> host_tables;  // (and the target of the result's D2H copies)
  Scratch scratch(ctx, st);

  // ---- stage 1: the WHERE clause's doc bitmap per segment where it neither matches all nor is empty
  std::vector<WhereBitmap> bitmap((size_t)nseg);
  for (int i = 0; i < nseg; ++i)
    if (cls[i] != FP_EMPTY && cls[i] != FP_ALL) bitmap[i] = where_bitmap(ctx, q, q->filter_root, segs[i], scratch, dev_ms);
  check_interrupt(q);

  // ---- time ranks: per time column the sorted distinct (long) times over the scanned segments
  auto scanned = [&](int i) { return cls[i] != FP_EMPTY && segs[i]->num_docs != 0; };
  std::vector<const int64_t*> d_times(time_cols.size(), nullptr);
  for (size_t t = 0; t < time_cols.size(); ++t) {
    std::vector<int64_t>& v = times[t];
    for (int i = 0; i < nseg; ++i) {
      if (!scanned(i)) continue;
      const Column& c = *segs[i]->columns.at(time_cols[t]);
      for (int32_t id = 0; id < c.cardinality; ++id) v.push_back(time_of(c, id));
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    if (v.size() >= 0xFFFFFFFFull) fail(PH_ERR_UNSUPPORTED, "with-time functions over 2^32 - 1 distinct times or more");
    if (v.empty()) continue;
    int64_t* dt = scratch.alloc<int64_t>(v.size());
    PH_HIP_CHECK(hipMemcpyAsync(dt, v.data(), 8 * v.size(), hipMemcpyHostToDevice, st));
    d_times[t] = dt;
  }

  // ---- stage 2: device segments (with each slot's hi_of table), chunks, tables
  int max_bits = 0;
  std::vector<int32_t> max_card((size_t)ns, 1);
  uint32_t base = 0;
  for (int i = 0; i < nseg; ++i) {
    if (!scanned(i)) continue;
    WSegment d{};
    WFinSeg f{};
    d.num_docs = f.num_docs = segs[i]->num_docs;
    f.base = base;
    d.lo_base = 0xFFFFFFFFu - (base + (uint32_t)d.num_docs - 1u);
    base += (uint32_t)d.num_docs;
    d.mask = bitmap[i].words;
    group_streams(ks, segs[i], d.gfwd, d.gbits, d.gremap, scratch, remap_keep, st);
    for (int v = 0; v < ns; ++v) {
      const Slot& s = slots[(size_t)v];
      const Column& c = *segs[i]->columns.at(s.tcol);
      if (!c.d_fwd.ptr) fail(PH_ERR_UNSUPPORTED, "with-time column " + s.tcol + " has no forward index");
      const std::vector<int64_t>& rank_of = times[(size_t)s.tc];
      const uint32_t T = (uint32_t)rank_of.size();
      std::vector<uint32_t> tab((size_t)std::max(1, c.cardinality), 1u);
      for (int32_t id = 0; id < c.cardinality; ++id) {
        const uint32_t rank = (uint32_t)(std::lower_bound(rank_of.begin(), rank_of.end(), time_of(c, id)) - rank_of.begin());
        tab[(size_t)id] = s.first ? T - rank : rank + 1u;
      }
      uint32_t* dt = scratch.alloc<uint32_t>(tab.size());
      hi_keep.push_back(std::move(tab));
      PH_HIP_CHECK(hipMemcpyAsync(dt, hi_keep.back().data(), 4 * hi_keep.back().size(), hipMemcpyHostToDevice, st));
      d.tfwd[v] = c.d_fwd.as<uint32_t>();
      d.hi_of[v] = dt;
      d.tbits[v] = c.bits;
      d.card[v] = std::max(1, c.cardinality);
      max_bits = std::max(max_bits, (int)c.bits);
      max_card[(size_t)v] = std::max(max_card[(size_t)v], d.card[v]);
    }
    for (int w = 0; w < nw; ++w) {
      const Column& c = *segs[i]->columns.at(waggs[(size_t)w].dcol);
      if (!c.d_fwd.ptr || !c.d_values.ptr) fail(PH_ERR_UNSUPPORTED, "with-time column " + waggs[(size_t)w].dcol + " has no dictionary table");
      f.dfwd[w] = c.d_fwd.as<uint32_t>();
      f.dvals[w] = c.d_values.ptr;
      f.dbits[w] = c.bits;
      f.dcard[w] = std::max(1, c.cardinality);
      const bool col_int = c.data_type == PH_INT || c.data_type == PH_LONG;
      const int32_t declared = waggs[(size_t)w].declared;
      f.dkind[w] = (declared == PH_INT || declared == PH_LONG) ? WT_I64
                   : (col_int ? WT_F64_OF_I64 : (declared == PH_FLOAT ? WT_F64_OF_F32 : WT_F64));
    }
    append_chunks(chunks, (int32_t)wsegs.size(), d.num_docs);
    wsegs.push_back(d);
    fsegs.push_back(f);
  }
  // u64 units: [segments] matched docs | the cells [G][ns] | n[G] | per with-time aggregation its pairs [G][2]
  const size_t nbs = wsegs.size();
  const size_t cnt_cells = std::max<size_t>(1, nbs);
  const size_t n_off = cnt_cells + (size_t)G * (size_t)ns;
  const size_t out_off = n_off + (size_t)G;
  const size_t words = out_off + (size_t)G * 2 * (size_t)nw;
  // the host copy holds the counters, n and the pairs (not the cells); no launch leaves n zero and the default pairs
  const size_t host_n = cnt_cells, host_out = cnt_cells + (size_t)G;
  host_tables.assign(host_out + (size_t)G * 2 * (size_t)nw, 0ull);
  for (int w = 0; w < nw; ++w) {
    WFinAgg& a = faggs[(size_t)w];
    const Slot& s = slots[(size_t)waggs[(size_t)w].slot];
    a.slot = waggs[(size_t)w].slot;
    a.first = s.first;
    default_pair(waggs[(size_t)w].declared, s.first, &a.default_value, &a.default_time);
    a.time_of_rank = d_times[(size_t)s.tc];
    a.num_times = (int64_t)times[(size_t)s.tc].size();
    if (chunks.empty())
      for (int64_t g = 0; g < G; ++g) {
        memcpy(&host_tables[host_out + 2 * ((size_t)G * (size_t)w + (size_t)g)], &a.default_value, 8);
        memcpy(&host_tables[host_out + 2 * ((size_t)G * (size_t)w + (size_t)g) + 1], &a.default_time, 8);
      }
  }
  if (!chunks.empty()) {
    unsigned long long* tables = scratch.alloc<unsigned long long>(words);
    WSegment* d_segs = scratch.alloc<WSegment>(nbs);
    WFinSeg* d_fsegs = scratch.alloc<WFinSeg>(nbs);
    WFinAgg* d_faggs = scratch.alloc<WFinAgg>((size_t)nw);
    Chunk* d_chunks = scratch.alloc<Chunk>(chunks.size());
    for (int w = 0; w < nw; ++w) faggs[(size_t)w].out = reinterpret_cast<int64_t*>(tables + out_off) + (size_t)G * 2 * (size_t)w;
    PH_HIP_CHECK(hipMemcpyAsync(d_segs, wsegs.data(), sizeof(WSegment) * nbs, hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipMemcpyAsync(d_fsegs, fsegs.data(), sizeof(WFinSeg) * nbs, hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipMemcpyAsync(d_faggs, faggs.data(), sizeof(WFinAgg) * (size_t)nw, hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), sizeof(Chunk) * chunks.size(), hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_start, st));
    PH_HIP_CHECK(hipMemsetAsync(tables, 0, 8 * out_off, st));
    WParams wp{};
    wp.segs = d_segs;
    wp.chunks = d_chunks;
    wp.chunk_end = (int32_t)chunks.size();
    wp.num_slots = ns;
    wp.num_group_cols = (int32_t)group_cols.size();
    std::copy(ks.stride, ks.stride + kMaxGroupCols, wp.group_stride);
    wp.num_groups = G;
    wp.combine_rounds = ctx->has(OPT_WITHTIME_NO_COMBINE) ? 0 : kWMatchRounds;
    wp.cells = tables + cnt_cells;
    wp.n = counting ? tables + n_off : nullptr;
    wp.seg_count = tables;
    // the hi_of tables go to LDS when every slot's largest table fits the budget together (16-byte aligned each)
    int64_t tab_budget = 32 * 1024;
    if (ctx->has(OPT_WITHTIME_TABLE_LDS_MAX)) tab_budget = std::max<int64_t>(0, ctx->opt(OPT_WITHTIME_TABLE_LDS_MAX));
    int64_t tab_u32 = 0;
    for (int v = 0; v < ns; ++v) {
      wp.tab_off[v] = (int32_t)tab_u32;
      tab_u32 += ((int64_t)max_card[(size_t)v] + 3) / 4 * 4;
    }
    wp.tab_lds = 4 * tab_u32 <= std::min<int64_t>(tab_budget, 64 * 1024);
    wp.tab_bytes = wp.tab_lds ? (int32_t)(4 * tab_u32) : 0;
    // (MODE_GROUP_LDS was chosen on the cells alone: with the staged tables they may not fit)
    if (mode == MODE_GROUP_LDS && withtime_lds_bytes(wp, mode) > 160 * 1024) {
      wp.tab_lds = 0;
      wp.tab_bytes = 0;
    }
    WFinishParams fin{};
    fin.num_groups = G;
    fin.num_aggs = nw;
    fin.num_slots = ns;
    fin.num_segs = (int32_t)nbs;
    fin.write_n = !counting;
    fin.cells = wp.cells;
    fin.n = tables + n_off;
    fin.segs = d_fsegs;
    fin.aggs = d_faggs;
    const bool reg = mode == MODE_AGG && max_bits <= 16;
    launch_scan_withtime(wp, mode, reg, scan_grid(ctx, mode, chunks.size()), st);
    launch_withtime_finish(fin, st);
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_stop, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data(), tables, 8 * cnt_cells, hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data() + host_n, tables + n_off, 8 * (words - n_off), hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0.f;
    PH_HIP_CHECK(hipEventElapsedTime(&ms, lane.lane->ev_start, lane.lane->ev_stop));
    dev_ms += (double)ms;
  }
  stats.scan_kernel = PH_KERNEL_SCAN_WITHTIME;

  // ---- statistics (docs x the group-by columns and the distinct data and time columns, as the reference projects
  // them); result rows: a group is a row when it holds a doc; an aggregation-only query has one row, the default pairs
  // where nothing matched
  add_scan_stats(stats, host_tables.data(), nbs, (int64_t)group_cols.size() + (int64_t)proj_cols.size(), bitmap);
  emit_rows(res.get(), q, ks, host_tables.data() + host_n, agg_w,
            reinterpret_cast<const uint8_t*>(host_tables.data() + host_out), (size_t)16);
  finish_result(res.get(), mode, dev_ms, t0);
  return res.release();
}

}  // namespace ph
