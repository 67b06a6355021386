// bins.cpp -- host-side plan of HISTOGRAM (the reference's HistogramAggregationFunction), alone or beside COUNT(*), with
// or without a WHERE clause and a GROUP BY.
//
// The reference adds 1.0 at getBinId(value) of a DoubleArrayList per result holder (HistogramAggregationFunction.java:
// 117-141, 191-298).  The bin of a doc depends on its dictionary value only, so this plan evaluates getBinId once per
// dictionary entry here, in doubles, exactly as Java does, into a uint16 table bin_of[dictId] per (segment, slot) with
// the invalid bin mapped to index B; the scan (scan_bins.hip) counts B + 1 uint32 cells per (row, slot) and
// k_bins_finish turns them into the row's matched docs and its B counts as doubles.  A slot is one distinct (column,
// edges) pair of the query; aggregations with the same pair share it.
//
// Stage 1, the key space, the mode rule, the statistics and the assembly of the result are the shared steps of
// scan_plan.h; the slots' tuples have their own widths (8 B bytes), which emit_rows takes per slot.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>

#include "scan_plan.h"

namespace ph {

namespace {

constexpr Family kFamily{"histogram", "histograms"};
constexpr int32_t kBadBin = -2;  // Java would index its DoubleArrayList out of bounds

struct Slot {
  std::string col;
  std::vector<double> edges;
  int32_t equal = 0;
  int32_t bins = 0;
};

// (int) of a double as Java casts it: NaN is 0, the rest saturates
int32_t java_int(double x) {
  if (std::isnan(x)) return 0;
  if (x >= 2147483647.0) return INT32_MAX;
  if (x <= -2147483648.0) return INT32_MIN;
  return (int32_t)x;
}

// the edges as the reference's constructor accepts them (HistogramAggregationFunction.java:52-110); returns B
int32_t check_edges(const double* edges, int32_t ne, int32_t equal) {
  if (!edges) fail(PH_ERR_BAD_QUERY, "HISTOGRAM without bin edges");
  if (equal < 0) fail(PH_ERR_BAD_QUERY, "The number of bins must be greater than zero, given " + std::to_string(equal));
  if (equal > 0) {
    if (ne != 2) fail(PH_ERR_BAD_QUERY, "HISTOGRAM with equal-length bins takes {lower, upper}");
    if (!(edges[1] > edges[0])) fail(PH_ERR_BAD_QUERY, "The right most edge must be greater than left most edge");
    return equal;
  }
  if (ne < 2) fail(PH_ERR_BAD_QUERY, "The number of bin edges must be greater than 1");
  for (int32_t i = 1; i < ne; ++i)
    if (!(edges[i] > edges[i - 1])) fail(PH_ERR_BAD_QUERY, "The bin edges must be strictly increasing");
  return ne - 1;
}

// getBinId (:117-141): -1 outside every bin, kBadBin where Java's list index would be out of bounds
int32_t bin_id(const double* edges, int32_t ne, int32_t equal, double val) {
  const double lower = edges[0], upper = edges[ne - 1];
  const int32_t B = equal > 0 ? equal : ne - 1;
  if (val > upper || val < lower) return -1;
  if (val == upper) return B - 1;
  int32_t id;
  if (equal > 0) {
    const double bin_length = (upper - lower) / equal;
    id = java_int(std::floor((val - lower) / bin_length));
  } else {
    int32_t i = 0, j = ne - 1;
    while (i < j) {
      const int32_t mid = (i + j + 1) / 2;
      if (edges[mid] > val) j = mid - 1;
      else i = mid;
    }
    id = i;
  }
  return (id < 0 || id >= B) ? kBadBin : id;
}

double stored_value(int32_t data_type, const void* values, int64_t i) {
  switch (data_type) {
    case PH_INT: return (double)static_cast<const int32_t*>(values)[i];
    case PH_LONG: return (double)static_cast<const int64_t*>(values)[i];
    case PH_FLOAT: return (double)static_cast<const float*>(values)[i];
    case PH_DOUBLE: return static_cast<const double*>(values)[i];
    default: fail(PH_ERR_UNSUPPORTED, "histogram function on STRING values");
  }
}

const ph_histogram_args& args_of(const ph_query* q, int k) {
  if (!q->histograms) fail(PH_ERR_BAD_QUERY, "HISTOGRAM without bin edges (ph_query.histograms)");
  return q->histograms[k];
}

}  // namespace

void histogram_bin_ids(const double* edges, int32_t num_edges, int32_t equal_bins, int32_t data_type, const void* values,
                       int64_t count, int32_t* out) {
  check_edges(edges, num_edges, equal_bins);
  if (count < 0 || (count > 0 && (!values || !out))) fail(PH_ERR_INVALID_ARGUMENT, "null argument");
  for (int64_t i = 0; i < count; ++i) {
    const int32_t b = bin_id(edges, num_edges, equal_bins, stored_value(data_type, values, i));
    if (b == kBadBin)
      fail(PH_ERR_UNSUPPORTED, "HISTOGRAM value whose bin the reference indexes out of bounds (a NaN, or an equal-length "
                               "bin id that reaches the number of bins)");
    out[i] = b;
  }
}

bool has_histogram_aggregation(const ph_query* q) {
  if (!q || !q->aggregations) return false;
  for (int k = 0; k < q->num_aggregations; ++k)
    if (q->aggregations[k].type == PH_AGG_HISTOGRAM) return true;
  return false;
}

void bins_validate(const ph_query* q) {
  check_query(q);
  for (int k = 0; k < q->num_aggregations; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    refuse_plain_beside(kFamily, a);
    if (is_moment(a.type)) fail(PH_ERR_UNSUPPORTED, "variance function beside a histogram function");
    if (is_comoment(a.type)) fail(PH_ERR_UNSUPPORTED, "covariance function beside a histogram function");
    if (is_moment4(a.type)) fail(PH_ERR_UNSUPPORTED, "fourth-moment function beside a histogram function");
    if (a.type != PH_AGG_COUNT && a.type != PH_AGG_HISTOGRAM) fail(PH_ERR_UNSUPPORTED, "aggregation type");
    if (a.filter) fail(PH_ERR_UNSUPPORTED, "a FILTER clause on or beside a histogram function");
    if (a.type == PH_AGG_COUNT) continue;
    if (a.expr_op != PH_EXPR_NONE) fail(PH_ERR_UNSUPPORTED, "histogram function of a 2-operand expression");
    if (!a.column) fail(PH_ERR_BAD_QUERY, "aggregation needs a column");
    const ph_histogram_args& h = args_of(q, k);
    if (check_edges(h.hist_edges, h.hist_num_edges, h.hist_equal_bins) > kBMaxBins)
      fail(PH_ERR_UNSUPPORTED, "histogram function with more than " + std::to_string(kBMaxBins) + " bins");
  }
  check_shape(kFamily, q);
}

ph_result* bins_execute(Context* ctx, const ph_query* q, ph_segment* const* segs_in, int32_t nseg) {
  const auto t0 = std::chrono::steady_clock::now();
  bins_validate(q);
  const std::vector<ph_segment*> segs = check_call(ctx, q, segs_in, nseg);

  // ---- slots (one per distinct (column, edges) pair), columns, the call's docs
  const int nagg = q->num_aggregations;
  std::vector<Slot> slots;
  std::vector<int> agg_slot(nagg, -1);
  for (int k = 0; k < nagg; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.type == PH_AGG_COUNT) continue;
    const ph_histogram_args& h = q->histograms[k];
    Slot s;
    s.col = a.column;
    s.edges.assign(h.hist_edges, h.hist_edges + h.hist_num_edges);
    s.equal = h.hist_equal_bins;
    s.bins = s.equal > 0 ? s.equal : h.hist_num_edges - 1;
    size_t at = 0;
    // (bitwise: -0.0 and 0.0 as edges are different argument lists, and give the same bins)
    while (at < slots.size() && !(slots[at].col == s.col && slots[at].equal == s.equal &&
                                  slots[at].edges.size() == s.edges.size() &&
                                  !memcmp(slots[at].edges.data(), s.edges.data(), 8 * s.edges.size())))
      ++at;
    if (at == slots.size()) slots.push_back(std::move(s));
    agg_slot[k] = (int)at;
  }
  const int ns = (int)slots.size();
  if (ns > kBMaxSlots)
    fail(PH_ERR_UNSUPPORTED, "more than " + std::to_string(kBMaxSlots) + " distinct (column, bins) pairs under histogram functions");
  const std::vector<std::string> group_cols = group_columns(q);
  check_columns(q, segs, group_cols);
  double docs_queried = 0.0;
  for (auto* s : segs) docs_queried += (double)s->num_docs;
  if (docs_queried >= 4294967296.0) fail(PH_ERR_UNSUPPORTED, "histograms over a call of 2^32 docs or more");
  std::vector<std::string> arg_cols;  // distinct argument columns (the statistic's projected columns)
  size_t row_cells = 0, row_bins = 0;
  std::vector<size_t> slot_bytes((size_t)ns);
  for (int v = 0; v < ns; ++v) {
    numeric_range(kFamily, slots[(size_t)v].col, segs);  // refuses STRING, sketch and mixed-type columns
    if (std::find(arg_cols.begin(), arg_cols.end(), slots[(size_t)v].col) == arg_cols.end())
      arg_cols.push_back(slots[(size_t)v].col);
    row_cells += (size_t)slots[(size_t)v].bins + 1;
    row_bins += (size_t)slots[(size_t)v].bins;
    slot_bytes[(size_t)v] = 8 * (size_t)slots[(size_t)v].bins;
  }

  // ---- the WHERE clause's class per segment, the key space, the mode
  std::vector<int32_t> cls((size_t)nseg);
  for (int i = 0; i < nseg; ++i) cls[i] = where_class(q, segs[i]);
  const KeySpace ks = key_space(kFamily, group_cols, segs);
  const int64_t G = ks.G;
  refuse_group_limit(kFamily, q, ks, segs, cls);
  // tables: the cells, n and the counts as doubles
  const int mode = choose_mode(ctx, kFamily, ks, (double)G * (4.0 * (double)row_cells + 8.0 + 8.0 * (double)row_bins),
                               (double)G * 4.0 * (double)row_cells);

  auto res = new_result(ctx, segs);
  ph_exec_stats& stats = res->stats;
  double dev_ms = 0.0;

  LaneGuard lane(ctx);
  const hipStream_t st = lane.stream();
  // host sources of the stream's H2D copies: declared before `scratch`, whose destructor drains the stream, so they
  // outlive every copy also when the call unwinds by a throw
  std::vector<BSegment> bsegs;
  std::vector<Chunk> chunks;
  std::vector<std::vector<int32_t>> remap_keep;
  std::vector<std::vector<uint16_t>> bin_of_keep;
  std::vector<unsigned long long> host_tables;  // (and the target of the result's D2H copies)
  Scratch scratch(ctx, st);

  // ---- stage 1: the WHERE clause's doc bitmap per segment where it neither matches all nor is empty
  std::vector<WhereBitmap> bitmap((size_t)nseg);
  for (int i = 0; i < nseg; ++i)
    if (cls[i] != FP_EMPTY && cls[i] != FP_ALL) bitmap[i] = where_bitmap(ctx, q, q->filter_root, segs[i], scratch, dev_ms);
  check_interrupt(q);

  // ---- stage 2: device segments (with each slot's bin_of table), chunks, tables
  int max_bits = 0;
  std::vector<int32_t> max_card((size_t)ns, 1);
  for (int i = 0; i < nseg; ++i) {
    if (cls[i] == FP_EMPTY || segs[i]->num_docs == 0) continue;
    BSegment d{};
    d.num_docs = segs[i]->num_docs;
    d.mask = bitmap[i].words;
    group_streams(ks, segs[i], d.gfwd, d.gbits, d.gremap, scratch, remap_keep, st);
    for (int v = 0; v < ns; ++v) {
      const Slot& s = slots[(size_t)v];
      const Column& c = *segs[i]->columns.at(s.col);
      if (!c.d_fwd.ptr) fail(PH_ERR_UNSUPPORTED, "histogram column " + s.col + " has no forward index");
      const bool is_int = c.data_type == PH_INT || c.data_type == PH_LONG;
      std::vector<uint16_t> tab((size_t)std::max(1, c.cardinality), (uint16_t)s.bins);
      for (int32_t id = 0; id < c.cardinality; ++id) {
        // the stored value as a double first: (double) of the int64 for LONG, FLOAT already widened
        const double val = is_int ? (double)c.dict.ints[(size_t)id] : c.dict.reals[(size_t)id];
        const int32_t b = bin_id(s.edges.data(), (int32_t)s.edges.size(), s.equal, val);
        if (b == kBadBin)
          fail(PH_ERR_UNSUPPORTED, "histogram column " + s.col + " holds a value whose bin the reference indexes out of "
                                   "bounds (a NaN, or an equal-length bin id that reaches the number of bins)");
        tab[(size_t)id] = (uint16_t)(b < 0 ? s.bins : b);
      }
      uint16_t* dt = scratch.alloc<uint16_t>(tab.size());
      bin_of_keep.push_back(std::move(tab));
      PH_HIP_CHECK(hipMemcpyAsync(dt, bin_of_keep.back().data(), 2 * bin_of_keep.back().size(), hipMemcpyHostToDevice, st));
      d.vfwd[v] = c.d_fwd.as<uint32_t>();
      d.bin_of[v] = dt;
      d.vbits[v] = c.bits;
      d.card[v] = std::max(1, c.cardinality);
      max_bits = std::max(max_bits, (int)c.bits);
      max_card[(size_t)v] = std::max(max_card[(size_t)v], d.card[v]);
    }
    append_chunks(chunks, (int32_t)bsegs.size(), d.num_docs);
    bsegs.push_back(d);
  }
  // u64 units: [segments] matched docs | the cells, u32 [G][row_cells] | n[G] | per slot its counts, double [G][B]
  const size_t nbs = bsegs.size();
  const size_t cnt_cells = std::max<size_t>(1, nbs);
  const size_t cell_words = ((size_t)G * row_cells + 1) / 2;
  const size_t n_off = cnt_cells + cell_words;
  const size_t out_off = n_off + (size_t)G;
  const size_t words = out_off + (size_t)G * row_bins;
  // the host copy holds the counters, n and the counts (not the cells); no launch leaves it zero: no row, or B zeros
  const size_t host_n = cnt_cells, host_out = cnt_cells + (size_t)G;
  host_tables.assign(host_out + (size_t)G * row_bins, 0ull);
  if (!chunks.empty()) {
    unsigned long long* tables = scratch.alloc<unsigned long long>(words);
    BSegment* d_segs = scratch.alloc<BSegment>(nbs);
    Chunk* d_chunks = scratch.alloc<Chunk>(chunks.size());
    PH_HIP_CHECK(hipMemcpyAsync(d_segs, bsegs.data(), sizeof(BSegment) * nbs, hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), sizeof(Chunk) * chunks.size(), hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_start, st));
    PH_HIP_CHECK(hipMemsetAsync(tables, 0, 8 * n_off, st));
    BParams bp{};
    bp.segs = d_segs;
    bp.chunks = d_chunks;
    bp.chunk_end = (int32_t)chunks.size();
    bp.num_slots = ns;
    bp.num_group_cols = (int32_t)group_cols.size();
    std::copy(ks.stride, ks.stride + kMaxGroupCols, bp.group_stride);
    bp.num_groups = G;
    bp.row_cells = (int32_t)row_cells;
    bp.cells = reinterpret_cast<uint32_t*>(tables + cnt_cells);
    bp.seg_count = tables;
    BFinishParams fin{};
    fin.num_groups = G;
    fin.num_slots = ns;
    fin.row_cells = (int32_t)row_cells;
    fin.cells = bp.cells;
    fin.n = tables + n_off;
    // the bin tables go to LDS when every slot's largest table fits the budget together (16-byte aligned each)
    int64_t tab_budget = 32 * 1024;
    if (ctx->has(OPT_BINS_TABLE_LDS_MAX)) tab_budget = std::max<int64_t>(0, ctx->opt(OPT_BINS_TABLE_LDS_MAX));
    int32_t cell = 0;
    int64_t tab_u16 = 0, bin_at = 0;
    for (int v = 0; v < ns; ++v) {
      bp.bins[v] = fin.bins[v] = slots[(size_t)v].bins;
      bp.cell_off[v] = fin.cell_off[v] = cell;
      cell += slots[(size_t)v].bins + 1;
      bp.tab_off[v] = (int32_t)tab_u16;
      tab_u16 += ((int64_t)max_card[(size_t)v] + 7) / 8 * 8;
      fin.out[v] = reinterpret_cast<double*>(tables + out_off) + (size_t)G * (size_t)bin_at;
      bin_at += slots[(size_t)v].bins;
    }
    bp.tab_lds = 2 * tab_u16 <= std::min<int64_t>(tab_budget, 64 * 1024);
    bp.tab_bytes = bp.tab_lds ? (int32_t)(2 * tab_u16) : 0;
    int run_mode = mode;  // (MODE_GROUP_LDS was chosen on the counters alone: with the staged tables they may not fit)
    if (run_mode == MODE_GROUP_LDS && bins_lds_bytes(bp, run_mode) > 160 * 1024) {
      bp.tab_lds = 0;
      bp.tab_bytes = 0;
    }
    const bool reg = mode == MODE_AGG && max_bits <= 16;
    launch_scan_bins(bp, run_mode, reg, scan_grid(ctx, mode, chunks.size()), st);
    launch_bins_finish(fin, st);
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_stop, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data(), tables, 8 * cnt_cells, hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data() + host_n, tables + n_off, 8 * (words - n_off), hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0.f;
    PH_HIP_CHECK(hipEventElapsedTime(&ms, lane.lane->ev_start, lane.lane->ev_stop));
    dev_ms += (double)ms;
  }
  stats.scan_kernel = PH_KERNEL_SCAN_BINS;

  // ---- statistics (docs x the group-by and distinct argument columns); result rows: a group is a row when it holds a
  // doc, in a bin or not; an aggregation-only query has one row, B zeros where nothing matched
  add_scan_stats(stats, host_tables.data(), nbs, (int64_t)group_cols.size() + (int64_t)arg_cols.size(), bitmap);
  emit_rows(res.get(), q, ks, host_tables.data() + host_n, agg_slot,
            reinterpret_cast<const uint8_t*>(host_tables.data() + host_out), slot_bytes);
  finish_result(res.get(), mode, dev_ms, t0);
  return res.release();
}

}  // namespace ph
