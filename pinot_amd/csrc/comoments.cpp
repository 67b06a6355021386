// comoments.cpp -- host-side plan of COVAR_POP / COVAR_SAMP (the reference's CovarianceAggregationFunction), alone or
// beside COUNT(*), with or without a WHERE clause and a GROUP BY.
//
// The reference keeps a CovarianceTuple (sumX, sumY, sumXY, count) per result holder and adds every doc's x, y and x y
// in doubles (CovarianceAggregationFunction.java:95-140).  Here every ordered pair of argument columns (a slot) gets
// two shifts for the call, Kx and Ky: the smallest value of each column over the queried segments, read from the
// dictionaries' first entries.  dx = x - Kx and dy = y - Ky are unsigned, so every product is non-negative, and the scan
// (scan_comoments.hip) accumulates n, sum(dx), sum(dy) and sum(dx dy).  With rx, ry the ranges of the two columns and
// N the docs of the call's segments:
//   * both columns stored as INT or LONG, rx N < 2^64 and ry N < 2^64: the integer forms -- narrow when
//     rx ry N < 2^64 (sum(dx dy) is one u64 cell that never carries), wide when rx ry N < 2^128 (a (lo, hi) pair);
//   * a FLOAT / DOUBLE column in the pair, or integer columns past those bounds: the real form, the unshifted values and
//     the three sums in double (the tuple the reference ships is the unshifted sums: a shift would buy nothing).
// dx, dy (or the doubles) come from per-segment tables over the dictIds in per-call scratch.  k_comoments_finish then
// writes the tuple of every (group, slot); COVAR_POP and COVAR_SAMP over one pair share the slot and return the same
// tuple, (x, y) and (y, x) are two slots.
//
// Stage 1 and the group key space are the variance plan's (moments.cpp): a WHERE clause that neither matches all nor is
// empty on a segment runs through query_execute_impl's COUNT(*) + doc bitmap form and leaves the bitmap, its matched
// docs and its ordinary numEntriesScannedInFilter; group keys are the call's union-dictionary ids over one dense key
// space.  moments.cpp keeps those steps inline in moments_execute, so they are repeated here rather than shared.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "ph_internal.h"

namespace ph {

namespace {

bool is_comoment(int32_t t) { return t == PH_AGG_COVARPOP || t == PH_AGG_COVARSAMP; }
bool is_moment(int32_t t) { return t >= PH_AGG_VARPOP && t <= PH_AGG_STDDEVSAMP; }

struct Slot {
  std::string x, y;
  int form = CFORM_NARROW;
  int64_t kx = 0, ky = 0;  // the shifts (integer forms)
  bool x_int = true, y_int = true;
};

// one argument column over the call's segments: stored as an integer or not, and its smallest and largest value
struct ColRange {
  bool is_int = true, any = false;
  int64_t lo = 0, hi = 0;
};

ColRange column_range(const std::string& col, const std::vector<ph_segment*>& segs) {
  ColRange r;
  int col_int = -1;
  for (auto* seg : segs) {
    auto it = seg->columns.find(col);
    if (it == seg->columns.end()) fail(PH_ERR_BAD_QUERY, "Column not found: " + col + " in segment " + seg->name);
    const Column& c = *it->second;
    if (c.data_type == PH_STRING) fail(PH_ERR_UNSUPPORTED, "covariance function on STRING column " + col);
    if (c.sketch_words) fail(PH_ERR_UNSUPPORTED, "covariance function on sketch column " + col);
    const int ci = c.data_type == PH_INT || c.data_type == PH_LONG;
    if (col_int < 0) col_int = ci;
    else if (col_int != ci) fail(PH_ERR_UNSUPPORTED, "covariance column with mixed integer/real types across segments");
    if (c.cardinality <= 0 || !ci) continue;
    r.lo = r.any ? std::min(r.lo, c.dict.ints.front()) : c.dict.ints.front();
    r.hi = r.any ? std::max(r.hi, c.dict.ints.back()) : c.dict.ints.back();
    r.any = true;
  }
  r.is_int = col_int != 0;
  return r;
}

// the shifts and the form of one slot, from the two columns' ranges over the call's segments and the call's docs; the
// bounds are checked in 128-bit arithmetic
void plan_slot(Slot& s, const std::vector<ph_segment*>& segs, double docs_queried) {
  const ColRange x = column_range(s.x, segs), y = column_range(s.y, segs);
  s.x_int = x.is_int;
  s.y_int = y.is_int;
  s.form = CFORM_REAL;
  if (!x.is_int || !y.is_int) return;
  typedef unsigned __int128 u128;
  const u128 rx = (uint64_t)x.hi - (uint64_t)x.lo, ry = (uint64_t)y.hi - (uint64_t)y.lo;
  const u128 N = (uint64_t)std::max(1.0, docs_queried);
  const u128 max64 = ~(uint64_t)0, max128 = ~(u128)0;
  if (rx * N > max64 || ry * N > max64) return;  // (both factors below 2^64: the products fit 128 bits)
  s.kx = x.lo;
  s.ky = y.lo;
  const u128 rr = rx * ry;
  if (rr == 0 || rr <= max64 / N) s.form = CFORM_NARROW;
  else if (rr <= max128 / N) s.form = CFORM_WIDE;
}

}  // namespace

bool has_comoment_aggregation(const ph_query* q) {
  if (!q || !q->aggregations) return false;
  for (int k = 0; k < q->num_aggregations; ++k)
    if (is_comoment(q->aggregations[k].type)) return true;
  return false;
}

void comoments_validate(const ph_query* q) {
  if (!q) fail(PH_ERR_INVALID_ARGUMENT, "null query");
  if (q->num_aggregations < 0 || (q->num_aggregations > 0 && !q->aggregations))
    fail(PH_ERR_INVALID_ARGUMENT, "bad aggregation list");
  std::vector<std::pair<std::string, std::string>> pairs;
  for (int k = 0; k < q->num_aggregations; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.type >= PH_AGG_SUM && a.type <= PH_AGG_PERCENTILE) {
      static const char* fn[] = {"SUM", "MIN", "MAX", "DISTINCTCOUNTHLL", "DISTINCTCOUNT", "PERCENTILE"};
      fail(PH_ERR_UNSUPPORTED, std::string(fn[a.type - PH_AGG_SUM]) + " beside a covariance function");
    }
    // (the two plans use different shifts and cell sets: DESIGN.md, "Co-moments")
    if (is_moment(a.type)) fail(PH_ERR_UNSUPPORTED, "variance function beside a covariance function");
    if (a.type != PH_AGG_COUNT && !is_comoment(a.type)) fail(PH_ERR_UNSUPPORTED, "aggregation type");
    if (a.filter) fail(PH_ERR_UNSUPPORTED, "a FILTER clause on or beside a covariance function");
    if (a.type == PH_AGG_COUNT) continue;
    if (a.expr_op != PH_EXPR_NONE) fail(PH_ERR_UNSUPPORTED, "covariance function of an expression argument");
    // the reference takes arguments.get(0) and get(1) (CovarianceAggregationFunction.java:57-61): a call with one
    // argument fails there
    if (!a.column || !a.column2) fail(PH_ERR_BAD_QUERY, "a covariance function needs two columns");
    const std::pair<std::string, std::string> pr(a.column, a.column2);
    if (std::find(pairs.begin(), pairs.end(), pr) == pairs.end()) pairs.push_back(pr);
  }
  if ((int)pairs.size() > kCMaxSlots)
    fail(PH_ERR_UNSUPPORTED, "more than " + std::to_string(kCMaxSlots) + " distinct column pairs under covariance functions");
  if (q->num_aggregations > kMaxAggs) fail(PH_ERR_UNSUPPORTED, "too many aggregations");
  if (q->num_group_by > kMaxGroupCols) fail(PH_ERR_UNSUPPORTED, "too many group-by columns");
  if (q->min_segment_group_trim_size > 0 && q->num_group_by > 0 && q->num_order_by > 0)
    fail(PH_ERR_UNSUPPORTED, "covariance functions with segment group trim (minSegmentGroupTrimSize)");
}

ph_result* comoments_execute(Context* ctx, const ph_query* q, ph_segment* const* segs_in, int32_t nseg) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  comoments_validate(q);
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

  // ---- slots (one per ordered pair of argument columns), columns, the call's docs
  const int nagg = q->num_aggregations;
  std::vector<Slot> slots;
  std::vector<int> agg_slot(nagg, -1);
  for (int k = 0; k < nagg; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.type == PH_AGG_COUNT) continue;
    size_t at = 0;
    while (at < slots.size() && !(slots[at].x == a.column && slots[at].y == a.column2)) ++at;
    if (at == slots.size()) {
      slots.emplace_back();
      slots.back().x = a.column;
      slots.back().y = a.column2;
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
  int cell_bytes = 8;  // per key: n, then 24 bytes per narrow or real slot, 32 per wide one
  std::vector<std::string> arg_cols;  // the distinct argument columns (the statistics)
  for (auto& s : slots) {
    plan_slot(s, segs, docs_queried);
    cell_bytes += s.form == CFORM_WIDE ? 32 : 24;
    for (const std::string* c : {&s.x, &s.y})
      if (std::find(arg_cols.begin(), arg_cols.end(), *c) == arg_cols.end()) arg_cols.push_back(*c);
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
    if (segs.empty()) fail(PH_ERR_UNSUPPORTED, "covariance group-by without segments");
    gdicts.push_back(union_dictionary(g, segs));
    const int64_t sz = std::max<int64_t>(1, gdicts.back()->dict.size);
    if (G > (int64_t(1) << 40) / sz) fail(PH_ERR_UNSUPPORTED, "covariance functions over a group key space beyond the dense tables");
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
        fail(PH_ERR_UNSUPPORTED, "covariance functions where a segment could reach numGroupsLimit");
    }
  // n, four accumulator cells and the 32-byte tuple per slot (so G stays far below 2^32: the scan's keys are uint32)
  if ((double)G * (8.0 + 64.0 * ns) > kDenseTableBudget)
    fail(PH_ERR_UNSUPPORTED, "covariance functions over a group key space beyond the dense tables");
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
  std::vector<CSegment> msegs;
  std::vector<Chunk> chunks;
  std::vector<std::vector<int32_t>> remap_keep;
  std::vector<std::vector<uint64_t>> d_of_keep;
  std::vector<CSlot> launch_slots;
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

  // ---- stage 2: device segments (with each slot's two tables over the dictIds), chunks, tables
  std::vector<int> mseg_src;
  int max_bits = 1;
  for (int i = 0; i < nseg; ++i) {
    if (cls[i] == FP_EMPTY || segs[i]->num_docs == 0) continue;
    CSegment d{};
    d.num_docs = segs[i]->num_docs;
    d.mask = bitmap[i];
    for (size_t g = 0; g < group_cols.size(); ++g) {
      const Column& c = *segs[i]->columns.at(group_cols[g]);
      if (c.sketch_words || !c.d_fwd.ptr) fail(PH_ERR_UNSUPPORTED, "group-by column " + group_cols[g] + " has no forward index");
      d.gfwd[g] = c.d_fwd.as<uint32_t>();
      d.gbits[g] = c.bits;
      max_bits = std::max(max_bits, (int)c.bits);
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
      // dictId -> x - Kx as a u64 (integer forms), or the bits of (double) x
      auto table_of = [&](const std::string& col, bool is_int, int64_t shift, const uint32_t*& fwd, int32_t& bits) {
        const Column& c = *segs[i]->columns.at(col);
        if (!c.d_fwd.ptr) fail(PH_ERR_UNSUPPORTED, "covariance column " + col + " has no forward index");
        std::vector<uint64_t> tab((size_t)std::max(1, c.cardinality), 0);
        for (int32_t id = 0; id < c.cardinality; ++id) {
          if (s.form != CFORM_REAL) {
            tab[(size_t)id] = (uint64_t)c.dict.ints[(size_t)id] - (uint64_t)shift;
          } else {
            const double x = is_int ? (double)c.dict.ints[(size_t)id] : c.dict.reals[(size_t)id];
            memcpy(&tab[(size_t)id], &x, 8);
          }
        }
        unsigned long long* dt = scratch.alloc<unsigned long long>(tab.size());
        d_of_keep.push_back(std::move(tab));
        PH_HIP_CHECK(hipMemcpyAsync(dt, d_of_keep.back().data(), 8 * d_of_keep.back().size(), hipMemcpyHostToDevice, st));
        fwd = c.d_fwd.as<uint32_t>();
        bits = c.bits;
        max_bits = std::max(max_bits, (int)c.bits);
        return dt;
      };
      d.pair[v].x_of = table_of(s.x, s.x_int, s.kx, d.pair[v].xfwd, d.pair[v].xbits);
      d.pair[v].y_of = table_of(s.y, s.y_int, s.ky, d.pair[v].yfwd, d.pair[v].ybits);
    }
    const int32_t nw = (int32_t)(((int64_t)d.num_docs + 63) / 64);
    for (int32_t w = 0; w < nw; w += kChunkWords)
      chunks.push_back(Chunk{(int32_t)msegs.size(), w, std::min<int32_t>(nw, w + kChunkWords), 0});
    mseg_src.push_back(i);
    msegs.push_back(d);
  }
  // u64 cells: [segments] matched docs | n[G] | per slot S1x[G], S1y[G], Sxy lo[G], Sxy hi[G] | per slot the CTuple[G] of
  // the finish
  const size_t nms = msegs.size();
  const size_t cnt_cells = std::max<size_t>(1, nms);
  const size_t acc_cells = (size_t)G * (1 + 4 * (size_t)ns);
  const size_t out_off = cnt_cells + acc_cells;
  const size_t cells = out_off + 4 * (size_t)G * (size_t)ns;
  host_tables.assign(cells, 0ull);  // (a CTuple of zero bits is (0.0, 0.0, 0.0, 0))
  if (!chunks.empty()) {
    unsigned long long* tables = scratch.alloc<unsigned long long>(cells);
    CSegment* d_segs = scratch.alloc<CSegment>(nms);
    Chunk* d_chunks = scratch.alloc<Chunk>(chunks.size());
    CSlot* d_slots = scratch.alloc<CSlot>((size_t)ns);
    unsigned long long* n_tab = tables + cnt_cells;
    auto cell = [&](int slot, int which) { return n_tab + (size_t)G * (1 + 4 * (size_t)slot + (size_t)which); };
    // the launches' slots, grouped by form
    int form_begin[4] = {0, 0, 0, 0};
    for (int form = CFORM_NARROW; form <= CFORM_REAL; ++form) {
      for (int v = 0; v < ns; ++v)
        if (slots[(size_t)v].form == form) launch_slots.push_back(CSlot{v, cell(v, 0), cell(v, 1), cell(v, 2), cell(v, 3)});
      form_begin[form + 1] = (int)launch_slots.size();
    }
    PH_HIP_CHECK(hipMemcpyAsync(d_segs, msegs.data(), sizeof(CSegment) * nms, hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), sizeof(Chunk) * chunks.size(), hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipMemcpyAsync(d_slots, launch_slots.data(), sizeof(CSlot) * launch_slots.size(), hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_start, st));
    PH_HIP_CHECK(hipMemsetAsync(tables, 0, 8 * out_off, st));
    CFinishParams fin{};
    fin.num_groups = G;
    fin.num_slots = ns;
    fin.n = n_tab;
    for (int v = 0; v < ns; ++v) {
      fin.form[v] = slots[(size_t)v].form;
      fin.kx[v] = slots[(size_t)v].kx;
      fin.ky[v] = slots[(size_t)v].ky;
      fin.s1x[v] = cell(v, 0);
      fin.s1y[v] = cell(v, 1);
      fin.sxy[v] = cell(v, 2);
      fin.sxyhi[v] = cell(v, 3);
      fin.out[v] = reinterpret_cast<CTuple*>(tables + out_off + 4 * (size_t)G * (size_t)v);
    }
    const int per_cu = mode == MODE_GROUP_LDS ? 2 : 8;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)chunks.size(), (int64_t)ctx->num_cus * per_cu));
    // one launch per form among the slots; the first one counts the docs (n and the segments' matched docs)
    bool counted = false;
    for (int form = CFORM_NARROW; form <= CFORM_REAL; ++form) {
      CParams cp{};
      cp.segs = d_segs;
      cp.chunks = d_chunks;
      cp.slots = d_slots + form_begin[form];
      cp.num_slots = form_begin[form + 1] - form_begin[form];
      if (!cp.num_slots) continue;
      cp.chunk_end = (int32_t)chunks.size();
      cp.num_group_cols = (int32_t)group_cols.size();
      int64_t stride = 1;
      for (int g = (int)group_cols.size() - 1; g >= 0; --g) {
        cp.group_stride[g] = (uint32_t)stride;
        stride *= std::max<int64_t>(1, gdicts[(size_t)g]->dict.size);
      }
      cp.num_groups = G;
      if (!counted) {
        cp.n = n_tab;
        cp.seg_count = tables;
        counted = true;
      }
      launch_scan_comoments(cp, mode, form, max_bits, grid, st);
    }
    launch_comoments_finish(fin, st);
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_stop, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data(), tables, 8 * (cnt_cells + (size_t)G), hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data() + out_off, tables + out_off, 8 * (cells - out_off),
                                hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0.f;
    PH_HIP_CHECK(hipEventElapsedTime(&ms, lane.lane->ev_start, lane.lane->ev_stop));
    dev_ms += (double)ms;
  }
  stats.scan_kernel = PH_KERNEL_SCAN_COMOMENTS;
  const unsigned long long* seg_count = host_tables.data();
  const unsigned long long* n_host = host_tables.data() + cnt_cells;
  auto tuple_of = [&](int slot, int64_t g) {
    return reinterpret_cast<const uint8_t*>(host_tables.data() + out_off + 4 * ((size_t)G * (size_t)slot + (size_t)g));
  };

  // ---- statistics: matched docs, the WHERE clause's ordinary statistic, docs x projected columns
  const int64_t projected = (int64_t)(group_cols.size() + arg_cols.size());
  for (size_t d = 0; d < nms; ++d) {
    const int64_t docs = (int64_t)seg_count[d];
    stats.num_segments_matched += docs > 0;
    stats.num_docs_scanned += docs;
    stats.num_entries_scanned_post_filter += docs * projected;
  }
  for (int i = 0; i < nseg; ++i) stats.num_entries_scanned_in_filter += bm_entries[i];

  // ---- result rows: a group is a row when it holds a doc; an aggregation-only query has one row,
  // (0.0, 0.0, 0.0, 0) where nothing matched (CovarianceAggregationFunction.extractAggregationResult :155-162)
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
    const size_t width = count ? 8 : sizeof(CTuple);
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
