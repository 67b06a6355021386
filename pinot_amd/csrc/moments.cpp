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
// Stage 1 (a WHERE clause that neither matches all nor is empty on a segment becomes a doc bitmap), the dense key space
// of union-dictionary ids, the mode rule and the assembly of the result are the shared steps of scan_plan.h.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "scan_plan.h"

namespace ph {

namespace {

constexpr Family kFamily{"variance", "variance functions"};

struct Slot {
  std::string col;
  int form = MFORM_NARROW;
  int64_t shift = 0;  // K: an int64, or a double's bits (MFORM_REAL)
  bool is_int = true;
};

// the shift and the form of one slot, from the column's range over the call's segments and the call's docs
void plan_slot(Slot& s, const std::vector<ph_segment*>& segs, double docs_queried) {
  const NumericRange r = numeric_range(kFamily, s.col, segs);
  s.is_int = r.is_int;
  if (s.is_int) {
    const uint64_t half = ((uint64_t)r.ihi - (uint64_t)r.ilo) / 2;
    const int64_t K = (int64_t)((uint64_t)r.ilo + half);
    const uint64_t dmax = std::max((uint64_t)r.ihi - (uint64_t)K, (uint64_t)K - (uint64_t)r.ilo);
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
  }
  const double kd = 0.5 * r.lo + 0.5 * r.hi;
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
  check_query(q);
  std::vector<std::string> cols;
  for (int k = 0; k < q->num_aggregations; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    refuse_plain_beside(kFamily, a);
    if (a.type != PH_AGG_COUNT && !is_moment(a.type)) fail(PH_ERR_UNSUPPORTED, "aggregation type");
    if (a.filter) fail(PH_ERR_UNSUPPORTED, "a FILTER clause on or beside a variance function");
    if (a.type == PH_AGG_COUNT) continue;
    if (a.expr_op != PH_EXPR_NONE) fail(PH_ERR_UNSUPPORTED, "variance function of a 2-operand expression");
    if (!a.column) fail(PH_ERR_BAD_QUERY, "aggregation needs a column");
    if (std::find(cols.begin(), cols.end(), std::string(a.column)) == cols.end()) cols.push_back(a.column);
  }
  if ((int)cols.size() > kMMaxSlots)
    fail(PH_ERR_UNSUPPORTED, "more than " + std::to_string(kMMaxSlots) + " distinct columns under variance functions");
  check_shape(kFamily, q);
}

ph_result* moments_execute(Context* ctx, const ph_query* q, ph_segment* const* segs_in, int32_t nseg) {
  const auto t0 = std::chrono::steady_clock::now();
  moments_validate(q);
  const std::vector<ph_segment*> segs = check_call(ctx, q, segs_in, nseg);

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
  const std::vector<std::string> group_cols = group_columns(q);
  check_columns(q, segs, group_cols);
  double docs_queried = 0.0;
  for (auto* s : segs) docs_queried += (double)s->num_docs;
  int cell_bytes = 8;  // per key: n, then 16 bytes per narrow or real slot, 24 per wide one
  for (auto& s : slots) {
    plan_slot(s, segs, docs_queried);
    cell_bytes += s.form == MFORM_WIDE ? 24 : 16;
  }

  // ---- the WHERE clause's class per segment, the key space, the mode
  std::vector<int32_t> cls((size_t)nseg);
  for (int i = 0; i < nseg; ++i) cls[i] = where_class(q, segs[i]);
  const KeySpace ks = key_space(kFamily, group_cols, segs);
  const int64_t G = ks.G;
  refuse_group_limit(kFamily, q, ks, segs, cls);
  // tables: n, three accumulator cells and the 24-byte tuple per slot
  const int mode = choose_mode(ctx, kFamily, ks, (double)G * (8.0 + 48.0 * ns), (double)G * cell_bytes);

  auto res = new_result(ctx, segs);
  ph_exec_stats& stats = res->stats;
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
  std::vector<WhereBitmap> bitmap((size_t)nseg);
  for (int i = 0; i < nseg; ++i)
    if (cls[i] != FP_EMPTY && cls[i] != FP_ALL) bitmap[i] = where_bitmap(ctx, q, q->filter_root, segs[i], scratch, dev_ms);
  check_interrupt(q);

  // ---- stage 2: device segments (with each slot's d_of table), chunks, tables
  for (int i = 0; i < nseg; ++i) {
    if (cls[i] == FP_EMPTY || segs[i]->num_docs == 0) continue;
    MSegment d{};
    d.num_docs = segs[i]->num_docs;
    d.mask = bitmap[i].words;
    group_streams(ks, segs[i], d.gfwd, d.gbits, d.gremap, scratch, remap_keep, st);
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
    append_chunks(chunks, (int32_t)msegs.size(), d.num_docs);
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
    const int grid = scan_grid(ctx, mode, chunks.size());
    // one launch per form among the slots; the first one counts the docs (n and the segments' matched docs)
    bool counted = false;
    for (int form = MFORM_NARROW; form <= MFORM_REAL; ++form) {
      MParams mp{};
      mp.segs = d_segs;
      mp.chunks = d_chunks;
      mp.chunk_end = (int32_t)chunks.size();
      mp.num_group_cols = (int32_t)group_cols.size();
      std::copy(ks.stride, ks.stride + kMaxGroupCols, mp.group_stride);
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

  // ---- statistics (docs x the group-by and argument columns); result rows: a group is a row when it holds a doc; an
  // aggregation-only query has one row, (0, 0.0, 0.0) where nothing matched
  // (VarianceAggregationFunction.extractAggregationResult :190-197)
  add_scan_stats(stats, host_tables.data(), nms, (int64_t)group_cols.size() + ns, bitmap);
  emit_rows(res.get(), q, ks, host_tables.data() + cnt_cells, agg_slot,
            reinterpret_cast<const uint8_t*>(host_tables.data() + out_off), sizeof(MTuple));
  finish_result(res.get(), mode, dev_ms, t0);
  return res.release();
}

}  // namespace ph
