// filtered.cpp -- host-side plan of filtered aggregations: agg(...) FILTER(WHERE <filter>) for COUNT / SUM / MIN / MAX.
//
// Restates AggregationFunctionUtils.buildFilteredAggregateProjectOperators (pinot-core/.../aggregation/function/
// AggregationFunctionUtils.java:191-267) per segment:
//   * aggregations are grouped by structurally equal FilterContext (the HashMap at :210; FilterContext.equals compares
//     type, children in order and predicate, FilterContext.java:76-86): same_filter() below compares the subtrees, so
//     callers need not share root indices;
//   * main filter empty (:198-206): one pipeline over the (empty) main filter for every function;
//   * main filter matching all (:219-220): each sub-filter's own operator is the pipeline's filter -- also one that
//     matches all, which is then a pipeline of its own beside the unfiltered one;
//   * otherwise a sub-filter that is empty keeps its empty operator (:222-223), one that matches all hands its
//     functions to the unfiltered pipeline (:224-225, :243-245), and any other runs CombinedFilterOperator(main, sub);
//   * the unfiltered functions, if any, run over the main filter (:257-264).
// FilteredAggregationOperator.java:66-94 / FilteredGroupByOperator.java:107-190 run the pipelines one after another
// over one shared key space (:118-140) and add up their statistics (:89-91, :149-151).
//
// Stage 1 plans every filter exactly as a WHERE clause (query_execute_impl's COUNT(*) + doc bitmap form, the one
// ph_filter_execute drives) and leaves one doc bitmap per (segment, filter) in per-call scratch; stage 2 is one
// k_scan_filtered launch (scan_filtered.hip) that reads the group-by and value streams once.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <set>

#include "ph_internal.h"

namespace ph {

namespace {

std::string lit(const char* s) { return s ? std::string(s) : std::string(); }

const ph_filter_node& node_at(const ph_query* q, int32_t i) {
  if (i < 0 || i >= q->num_filter_nodes || !q->filter_nodes) fail(PH_ERR_INVALID_ARGUMENT, "bad filter node index");
  return q->filter_nodes[i];
}

// checks every node a root reaches (indices, types).  state: 0 unseen, 1 on the current path, 2 checked -- a node met
// again on its own path is a cycle; one already checked is not walked again, so shared subtrees cost one visit
void walk_tree(const ph_query* q, int32_t i, std::vector<char>& state, int depth) {
  const ph_filter_node& f = node_at(q, i);
  if (state[(size_t)i] == 1) fail(PH_ERR_INVALID_ARGUMENT, "filter nodes form a cycle");
  if (depth > 64) fail(PH_ERR_UNSUPPORTED, "filter tree too deep");
  if (state[(size_t)i] == 2) return;
  if (f.type == PH_FILTER_PREDICATE) {
    if (f.predicate < 0 || f.predicate >= q->num_predicates || !q->predicates)
      fail(PH_ERR_INVALID_ARGUMENT, "bad predicate index");
    state[(size_t)i] = 2;
    return;
  }
  if (f.type < PH_FILTER_AND || f.type > PH_FILTER_PREDICATE) fail(PH_ERR_INVALID_ARGUMENT, "bad filter node type");
  if (f.num_children < 0 || (f.num_children > 0 && !f.children)) fail(PH_ERR_INVALID_ARGUMENT, "bad filter children");
  state[(size_t)i] = 1;
  for (int k = 0; k < f.num_children; ++k) walk_tree(q, f.children[k], state, depth + 1);
  state[(size_t)i] = 2;
}

bool same_predicate(const ph_predicate& a, const ph_predicate& b) {
  if (a.type != b.type || lit(a.column) != lit(b.column)) return false;
  if (a.type == PH_PRED_RANGE)
    return lit(a.lower) == lit(b.lower) && lit(a.upper) == lit(b.upper) &&
           (a.lower_inclusive != 0) == (b.lower_inclusive != 0) && (a.upper_inclusive != 0) == (b.upper_inclusive != 0);
  if (a.num_values != b.num_values) return false;
  for (int i = 0; i < a.num_values; ++i)
    if (lit(a.values[i]) != lit(b.values[i])) return false;
  return true;
}

// FilterContext.equals: type, children in order, predicate
bool same_filter(const ph_query* q, int32_t a, int32_t b) {
  if (a == b) return true;
  const ph_filter_node &x = q->filter_nodes[a], &y = q->filter_nodes[b];
  if (x.type != y.type) return false;
  if (x.type == PH_FILTER_PREDICATE) return same_predicate(q->predicates[x.predicate], q->predicates[y.predicate]);
  if (x.num_children != y.num_children) return false;
  for (int k = 0; k < x.num_children; ++k)
    if (!same_filter(q, x.children[k], y.children[k])) return false;
  return true;
}

// per-call device buffers from the context's scratch pool, returned once the call's stream has drained
struct Scratch {
  Context* ctx;
  hipStream_t st;
  std::vector<std::unique_ptr<DeviceBuffer>> bufs;
  Scratch(Context* c, hipStream_t s) : ctx(c), st(s) {}
  ~Scratch() {
    (void)hipStreamSynchronize(st);
    for (auto& b : bufs) ctx->scratch_release(std::move(b));
  }
  template <class T>
  T* alloc(size_t count) {
    auto b = ctx->scratch_acquire(std::max<size_t>(16, sizeof(T) * count));
    T* p = b->as<T>();
    bufs.push_back(std::move(b));
    return p;
  }
};

void put_key(const Dictionary& d, int64_t id, uint8_t* dst, int32_t entry) {
  switch (d.type) {
    case PH_INT: { int32_t v = (int32_t)d.ints[(size_t)id]; memcpy(dst, &v, 4); break; }
    case PH_LONG: memcpy(dst, &d.ints[(size_t)id], 8); break;
    case PH_FLOAT: { float v = (float)d.reals[(size_t)id]; memcpy(dst, &v, 4); break; }
    case PH_DOUBLE: memcpy(dst, &d.reals[(size_t)id], 8); break;
    default:
      memset(dst, 0, (size_t)entry);
      memcpy(dst, d.strings[(size_t)id].data(), std::min<size_t>((size_t)entry, d.strings[(size_t)id].size()));
  }
}

int32_t entry_size_of(const Dictionary& d) {
  switch (d.type) {
    case PH_INT: case PH_FLOAT: return 4;
    case PH_LONG: case PH_DOUBLE: return 8;
    default: return std::max(1, d.max_string_len);
  }
}

}  // namespace

bool has_filtered_aggregation(const ph_query* q) {
  if (!q || !q->aggregations) return false;
  for (int k = 0; k < q->num_aggregations; ++k)
    if (q->aggregations[k].filter != 0) return true;
  return false;
}

std::string filter_to_string(const ph_query* q, int32_t root) {
  const ph_filter_node& f = node_at(q, root);
  auto join = [&](const char* sep) {
    if (f.num_children <= 0 || !f.children) fail(PH_ERR_INVALID_ARGUMENT, "filter node without children");
    std::string s = "(" + filter_to_string(q, f.children[0]);
    for (int i = 1; i < f.num_children; ++i) s += sep + filter_to_string(q, f.children[i]);
    return s + ")";
  };
  switch (f.type) {
    case PH_FILTER_AND: return join(" AND ");
    case PH_FILTER_OR: return join(" OR ");
    case PH_FILTER_NOT:
      if (f.num_children != 1 || !f.children) fail(PH_ERR_INVALID_ARGUMENT, "NOT needs exactly one child");
      return "(NOT " + filter_to_string(q, f.children[0]) + ")";
    case PH_FILTER_PREDICATE: break;
    default: fail(PH_ERR_INVALID_ARGUMENT, "bad filter node type");
  }
  if (f.predicate < 0 || f.predicate >= q->num_predicates || !q->predicates)
    fail(PH_ERR_INVALID_ARGUMENT, "bad predicate index");
  const ph_predicate& p = q->predicates[f.predicate];
  const std::string lhs = lit(p.column);
  auto list = [&](const char* kw) {  // In / NotInPredicate.toString (:58-66)
    std::string s = lhs + kw + "('";
    for (int i = 0; i < p.num_values; ++i) s += (i ? ",'" : "") + lit(p.values[i]) + "'";
    return s + ")";
  };
  switch (p.type) {
    case PH_PRED_EQ: return lhs + " = '" + (p.num_values > 0 ? lit(p.values[0]) : "") + "'";      // EqPredicate :64-66
    case PH_PRED_NOT_EQ: return lhs + " != '" + (p.num_values > 0 ? lit(p.values[0]) : "") + "'"; // NotEqPredicate :63-65
    case PH_PRED_IN: return list(" IN ");
    case PH_PRED_NOT_IN: return list(" NOT IN ");
    case PH_PRED_RANGE: {  // RangePredicate.toString (:122-134)
      const std::string lo = p.lower ? lit(p.lower) : "*", hi = p.upper ? lit(p.upper) : "*";
      if (lo == "*") return lhs + (p.upper_inclusive ? " <= '" : " < '") + hi + "'";
      if (hi == "*") return lhs + (p.lower_inclusive ? " >= '" : " > '") + lo + "'";
      if (p.lower_inclusive && p.upper_inclusive) return lhs + " BETWEEN '" + lo + "' AND '" + hi + "'";
      return "(" + lhs + (p.lower_inclusive ? " >= '" : " > '") + lo + "' AND " + lhs +
             (p.upper_inclusive ? " <= '" : " < '") + hi + "')";
    }
    default: fail(PH_ERR_UNSUPPORTED, "predicate type " + std::to_string(p.type) + " is not on the GPU path");
  }
}

void filtered_validate(const ph_query* q) {
  if (!q) fail(PH_ERR_INVALID_ARGUMENT, "null query");
  if (q->num_aggregations < 0 || (q->num_aggregations > 0 && !q->aggregations))
    fail(PH_ERR_INVALID_ARGUMENT, "bad aggregation list");
  const size_t nn = (size_t)std::max(0, q->num_filter_nodes);
  std::vector<char> state(nn, 0);
  if (q->filter_root >= 0) walk_tree(q, q->filter_root, state, 0);
  std::vector<int32_t> roots;
  for (int k = 0; k < q->num_aggregations; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.filter == 0) continue;
    const int32_t r = a.filter - 1;
    if (r < 0 || r >= q->num_filter_nodes) fail(PH_ERR_INVALID_ARGUMENT, "bad aggregation filter index");
    walk_tree(q, r, state, 0);
  }
  for (int k = 0; k < q->num_aggregations; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.type == PH_AGG_DISTINCTCOUNTHLL || a.type == PH_AGG_DISTINCTCOUNT || a.type == PH_AGG_PERCENTILE) {
      static const char* fn[] = {"DISTINCTCOUNTHLL", "DISTINCTCOUNT", "PERCENTILE"};
      fail(PH_ERR_UNSUPPORTED, std::string(fn[a.type - PH_AGG_DISTINCTCOUNTHLL]) +
                                   (a.filter ? " with a FILTER clause" : " beside filtered aggregations"));
    }
    if (a.type < PH_AGG_COUNT || a.type > PH_AGG_PERCENTILE) fail(PH_ERR_UNSUPPORTED, "aggregation type");
    if (a.expr_op != PH_EXPR_NONE)
      fail(PH_ERR_UNSUPPORTED, a.filter ? "FILTER clause on a 2-operand expression"
                                        : "2-operand expression beside filtered aggregations");
    if (a.filter) {
      const int32_t r = a.filter - 1;
      bool seen = false;
      for (int32_t x : roots) seen = seen || same_filter(q, x, r);
      if (!seen) roots.push_back(r);
    }
  }
  if ((int)roots.size() > kFMaxSubFilters)
    fail(PH_ERR_UNSUPPORTED, "more than " + std::to_string(kFMaxSubFilters) + " distinct FILTER clauses in one query");
  if (q->num_aggregations > kMaxAggs) fail(PH_ERR_UNSUPPORTED, "too many aggregations");
  if (q->num_group_by > kMaxGroupCols) fail(PH_ERR_UNSUPPORTED, "too many group-by columns");
  if (q->min_segment_group_trim_size > 0 && q->num_group_by > 0 && q->num_order_by > 0)
    fail(PH_ERR_UNSUPPORTED, "filtered aggregations with segment group trim (minSegmentGroupTrimSize)");
}

ph_result* filtered_execute(Context* ctx, const ph_query* q, ph_segment* const* segs_in, int32_t nseg) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  filtered_validate(q);
  if (nseg < 0 || (nseg > 0 && !segs_in)) fail(PH_ERR_INVALID_ARGUMENT, "bad segment list");
  std::vector<ph_segment*> segs(segs_in, segs_in + nseg);
  for (auto* s : segs)
    if (!s || s->ctx != ctx) fail(PH_ERR_INVALID_ARGUMENT, "segment is null or pinned on another context");
  auto check_interrupt = [&]() {
    if (q->interrupt && *q->interrupt) fail(PH_ERR_CANCELLED, "query interrupted");
    if (q->end_time_ms > 0) {
      const int64_t now = std::chrono::duration_cast<std::chrono::milliseconds>(
                              std::chrono::system_clock::now().time_since_epoch()).count();
      if (now > q->end_time_ms) fail(PH_ERR_CANCELLED, "query timed out (end time passed)");
    }
  };
  check_interrupt();

  // ---- pipelines, value terms and slots
  const int nagg = q->num_aggregations;
  std::vector<int32_t> sub_roots;            // distinct sub-filters; pipeline i + 1 is main AND sub_roots[i]
  std::vector<int> agg_pipe(nagg, 0), agg_slot(nagg, -1);
  bool has_unfiltered = false;
  for (int k = 0; k < nagg; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (!a.filter) { has_unfiltered = true; continue; }
    int at = -1;
    for (size_t i = 0; i < sub_roots.size(); ++i)
      if (same_filter(q, sub_roots[i], a.filter - 1)) { at = (int)i; break; }
    if (at < 0) { sub_roots.push_back(a.filter - 1); at = (int)sub_roots.size() - 1; }
    agg_pipe[k] = at + 1;
  }
  const int K = (int)sub_roots.size(), P = K + 1;
  std::vector<std::string> group_cols, val_cols;
  for (int g = 0; g < q->num_group_by; ++g) {
    if (!q->group_by || !q->group_by[g]) fail(PH_ERR_INVALID_ARGUMENT, "null group-by column");
    group_cols.push_back(q->group_by[g]);
  }
  std::vector<int> agg_val(nagg, -1);
  for (int k = 0; k < nagg; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.type == PH_AGG_COUNT) continue;
    if (!a.column) fail(PH_ERR_BAD_QUERY, "aggregation needs a column");
    auto it = std::find(val_cols.begin(), val_cols.end(), std::string(a.column));
    if (it == val_cols.end()) {
      if ((int)val_cols.size() >= kFMaxVals)
        fail(PH_ERR_UNSUPPORTED, "more than " + std::to_string(kFMaxVals) + " aggregated columns beside FILTER clauses");
      val_cols.push_back(a.column);
      agg_val[k] = (int)val_cols.size() - 1;
    } else {
      agg_val[k] = (int)(it - val_cols.begin());
    }
  }
  const int nvals = (int)val_cols.size();
  // columns exist (BadQueryRequestException otherwise), value columns are numeric and of one kind in every segment
  std::vector<int> val_is_int(nvals, 1), val_widened(nvals, 0);
  double docs_queried = 0.0;
  for (auto* s : segs) docs_queried += (double)s->num_docs;
  for (auto* s : segs) {
    for (auto& c : group_cols)
      if (!s->columns.count(c)) fail(PH_ERR_BAD_QUERY, "Column not found: " + c + " in segment " + s->name);
    for (int i = 0; i < q->num_predicates; ++i) {
      if (!q->predicates[i].column) fail(PH_ERR_BAD_QUERY, "predicate without column");
      if (!s->columns.count(q->predicates[i].column))
        fail(PH_ERR_BAD_QUERY, std::string("Column not found: ") + q->predicates[i].column);
    }
  }
  for (int j = 0; j < nvals; ++j) {
    int col_int = -1;
    double amax = 0.0;
    for (auto* s : segs) {
      auto it = s->columns.find(val_cols[j]);
      if (it == s->columns.end()) fail(PH_ERR_BAD_QUERY, "Column not found: " + val_cols[j] + " in segment " + s->name);
      const Column& c = *it->second;
      if (c.data_type == PH_STRING) fail(PH_ERR_UNSUPPORTED, "numeric aggregation on STRING column " + val_cols[j]);
      if (c.sketch_words) fail(PH_ERR_UNSUPPORTED, "sketch column " + val_cols[j] + " outside DISTINCTCOUNTHLL");
      const int ci = c.data_type == PH_INT || c.data_type == PH_LONG;
      if (col_int < 0) col_int = ci;
      else if (col_int != ci) fail(PH_ERR_UNSUPPORTED, "aggregation column with mixed integer/real types across segments");
      if (ci && c.cardinality > 0) {
        amax = std::max(amax, std::fabs((double)c.dict.ints.front()));
        amax = std::max(amax, std::fabs((double)c.dict.ints.back()));
      }
    }
    val_is_int[j] = col_int != 0;
    // the existing integer SUM contract: exact int64 while |term| x the call's docs stays below 2^63, else summed in
    // double as the reference does (SumAggregationFunction adds (double) value)
    bool sums = false;
    for (int k = 0; k < nagg; ++k) sums = sums || (agg_val[k] == j && q->aggregations[k].type == PH_AGG_SUM);
    if (val_is_int[j] && sums && amax * docs_queried >= 9.0e18) val_widened[j] = 1;
  }
  FParams fp{};
  int ns = 0;
  for (int k = 0; k < nagg; ++k) {
    const ph_aggregation& a = q->aggregations[k];
    if (a.type == PH_AGG_COUNT) continue;
    const int j = agg_val[k];
    int op;
    if (a.type == PH_AGG_SUM) op = val_is_int[j] ? (val_widened[j] ? FOP_SUM_I2F : FOP_SUM_I) : FOP_SUM_F;
    else if (a.type == PH_AGG_MIN) op = val_is_int[j] ? FOP_MIN_I : FOP_MIN_F;
    else op = val_is_int[j] ? FOP_MAX_I : FOP_MAX_F;
    int at = -1;
    for (int s = 0; s < ns; ++s)
      if (fp.slot_pipe[s] == agg_pipe[k] && fp.slot_op[s] == op && fp.slot_val[s] == j) at = s;
    if (at < 0) {
      at = ns++;  // (<= kMaxAggs == kFMaxSlots)
      fp.slot_pipe[at] = agg_pipe[k];
      fp.slot_op[at] = op;
      fp.slot_val[at] = j;
    }
    agg_slot[k] = at;
  }
  // the columns each pipeline projects: the group-by columns plus the argument columns of its functions
  // (AggregationFunctionUtils.collectExpressionsToTransform)
  auto projected = [&](const std::vector<char>& in_pipe) {
    std::set<std::string> cols(group_cols.begin(), group_cols.end());
    for (int k = 0; k < nagg; ++k)
      if (in_pipe[(size_t)agg_pipe[k]] && q->aggregations[k].column && q->aggregations[k].type != PH_AGG_COUNT)
        cols.insert(q->aggregations[k].column);
    return (int64_t)cols.size();
  };

  // ---- per segment: how main and every sub-filter plan (FilterPlanNode.run's isResultEmpty / isResultMatchingAll)
  std::vector<int32_t> main_cls(nseg, FP_ALL);
  std::vector<std::vector<int32_t>> sub_cls(nseg, std::vector<int32_t>((size_t)K, FP_ALL));
  for (int i = 0; i < nseg; ++i) {
    if (q->filter_root >= 0) main_cls[i] = filter_plan_class(q, q->filter_root, segs[i]);
    else if (segs[i]->num_docs == 0) main_cls[i] = FP_EMPTY;
    for (int f = 0; f < K; ++f) sub_cls[i][f] = filter_plan_class(q, sub_roots[f], segs[i]);
  }
  // a CombinedFilterOperator's statistic is derived for single-leaf sub-filters only
  for (int i = 0; i < nseg; ++i)
    for (int f = 0; f < K; ++f)
      if (main_cls[i] >= FP_SCAN_LEAF && sub_cls[i][f] == FP_COMPOSITE)
        fail(PH_ERR_UNSUPPORTED, "FILTER clause of several predicates (or over a legacy range index) under a WHERE clause");

  // ---- key space
  std::vector<std::shared_ptr<GlobalDict>> gdicts;
  int64_t G = 1;
  for (auto& g : group_cols) {
    if (segs.empty()) fail(PH_ERR_UNSUPPORTED, "filtered group-by without segments");
    gdicts.push_back(union_dictionary(g, segs));
    const int64_t sz = std::max<int64_t>(1, gdicts.back()->dict.size);
    if (G > (int64_t(1) << 40) / sz) fail(PH_ERR_UNSUPPORTED, "filtered aggregations over a group key space beyond the dense tables");
    G *= sz;
  }
  const int64_t group_limit = q->num_groups_limit > 0 ? q->num_groups_limit : 100000;
  if (!group_cols.empty())
    for (int i = 0; i < nseg; ++i) {
      if (main_cls[i] == FP_EMPTY) continue;
      int64_t pp = 1;
      for (auto& g : group_cols) {
        const int64_t c = std::max<int64_t>(1, segs[i]->columns.at(g)->cardinality);
        pp = pp > (int64_t(1) << 40) / c ? int64_t(1) << 40 : pp * c;
      }
      // past the limit the reference's group ids depend on the order of a HashMap over FilterContexts
      if (std::min<int64_t>(pp, segs[i]->num_docs) >= group_limit)
        fail(PH_ERR_UNSUPPORTED, "filtered aggregations where a segment could reach numGroupsLimit");
    }
  const double table_bytes = (double)G * 8.0 * (double)(P + ns);
  if (table_bytes > kDenseTableBudget)
    fail(PH_ERR_UNSUPPORTED, "filtered aggregations over a group key space beyond the dense tables");
  int mode = MODE_AGG;
  if (!group_cols.empty()) {
    size_t lds_table_max = 64 * 1024;
    if (ctx->has(OPT_LDS_TABLE_MAX)) lds_table_max = (size_t)std::max<int64_t>(0, ctx->opt(OPT_LDS_TABLE_MAX));
    lds_table_max = std::min<size_t>(lds_table_max, 160 * 1024);
    mode = table_bytes <= (double)lds_table_max ? MODE_GROUP_LDS : MODE_GROUP_GLOBAL;
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
  std::vector<FSegment> fsegs;
  std::vector<Chunk> chunks;
  std::vector<std::vector<int32_t>> remap_keep;
  std::vector<long long> host_tables;  // (and the target of the result's D2H copy)
  Scratch scratch(ctx, st);

  // ---- stage 1: one doc bitmap per (segment, filter that is neither empty nor matching all)
  struct Bitmap {
    unsigned long long* words = nullptr;
    int64_t docs = 0, entries = 0;  // matched docs; the filter's ordinary numEntriesScannedInFilter
  };
  auto run_filter = [&](int32_t root, ph_segment* seg) {
    Bitmap b;
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
  };
  std::vector<Bitmap> main_bm(nseg);
  std::vector<std::vector<Bitmap>> sub_bm(nseg, std::vector<Bitmap>((size_t)K));
  for (int i = 0; i < nseg; ++i) {
    if (main_cls[i] == FP_EMPTY) continue;
    if (main_cls[i] != FP_ALL) main_bm[i] = run_filter(q->filter_root, segs[i]);
    for (int f = 0; f < K; ++f)
      if (sub_cls[i][f] >= FP_SCAN_LEAF) sub_bm[i][f] = run_filter(sub_roots[f], segs[i]);
  }
  check_interrupt();

  // ---- stage 2: device segments, chunks, tables
  std::vector<int> fseg_src;
  for (int i = 0; i < nseg; ++i) {
    if (main_cls[i] == FP_EMPTY || segs[i]->num_docs == 0) continue;
    stats.num_segments_matched++;
    FSegment d{};
    d.num_docs = segs[i]->num_docs;
    for (int p = 0; p < P; ++p) {
      d.ma[p] = main_bm[i].words;  // nullptr: main matches all
      if (p == 0) {
        if (!has_unfiltered) d.empty |= 1u;
        continue;
      }
      const int32_t c = sub_cls[i][p - 1];
      if (c == FP_EMPTY) d.empty |= 1u << p;
      else if (c != FP_ALL) d.mb[p] = sub_bm[i][p - 1].words;
    }
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
    for (int v = 0; v < nvals; ++v) {
      const Column& c = *segs[i]->columns.at(val_cols[(size_t)v]);
      if (!c.d_fwd.ptr || !c.d_values.ptr) fail(PH_ERR_UNSUPPORTED, "value column " + val_cols[(size_t)v] + " has no dictionary table");
      d.vfwd[v] = c.d_fwd.as<uint32_t>();
      d.vtable[v] = c.d_values.ptr;
      d.vbits[v] = c.bits;
    }
    const int32_t nw = (int32_t)(((int64_t)d.num_docs + 63) / 64);
    for (int32_t w = 0; w < nw; w += kChunkWords)
      chunks.push_back(Chunk{(int32_t)fsegs.size(), w, std::min<int32_t>(nw, w + kChunkWords), 0});
    fseg_src.push_back(i);
    fsegs.push_back(d);
  }
  const size_t nfs = fsegs.size();
  const size_t cnt_cells = std::max<size_t>(1, nfs) * kFMaxPipes;
  const size_t pc_cells = mode == MODE_AGG ? 0 : (size_t)P * (size_t)G;
  const size_t cells = cnt_cells + pc_cells + (size_t)ns * (size_t)G;
  long long* tables = scratch.alloc<long long>(cells);
  host_tables.assign(cells, 0);
  if (!chunks.empty()) {
    FSegment* d_segs = scratch.alloc<FSegment>(nfs);
    Chunk* d_chunks = scratch.alloc<Chunk>(chunks.size());
    PH_HIP_CHECK(hipMemcpyAsync(d_segs, fsegs.data(), sizeof(FSegment) * nfs, hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), sizeof(Chunk) * chunks.size(), hipMemcpyHostToDevice, st));
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_start, st));
    PH_HIP_CHECK(hipMemsetAsync(tables, 0, 8 * (cnt_cells + pc_cells), st));
    fp.segs = d_segs;
    fp.chunks = d_chunks;
    fp.chunk_begin = 0;
    fp.chunk_end = (int32_t)chunks.size();
    fp.num_pipes = P;
    fp.num_slots = ns;
    fp.num_vals = nvals;
    fp.num_group_cols = (int32_t)group_cols.size();
    int64_t stride = 1;
    for (int g = (int)group_cols.size() - 1; g >= 0; --g) {
      fp.group_stride[g] = stride;
      stride *= std::max<int64_t>(1, gdicts[(size_t)g]->dict.size);
    }
    fp.num_groups = G;
    fp.seg_count = reinterpret_cast<unsigned long long*>(tables);
    fp.pcount = pc_cells ? reinterpret_cast<unsigned long long*>(tables + cnt_cells) : nullptr;
    for (int s = 0; s < ns; ++s) {
      fp.slot_out[s] = tables + cnt_cells + pc_cells + (size_t)s * (size_t)G;
      const int op = fp.slot_op[s];
      const int64_t idv = (op == FOP_MIN_I || op == FOP_MIN_F) ? INT64_MAX
                          : ((op == FOP_MAX_I || op == FOP_MAX_F) ? INT64_MIN : 0);
      launch_fill_i64(reinterpret_cast<int64_t*>(fp.slot_out[s]), idv, G, st);
    }
    const int per_cu = mode == MODE_GROUP_LDS ? 2 : 8;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)chunks.size(), (int64_t)ctx->num_cus * per_cu));
    launch_scan_filtered(fp, mode, grid, st);
    PH_HIP_CHECK(hipEventRecord(lane.lane->ev_stop, st));
    PH_HIP_CHECK(hipMemcpyAsync(host_tables.data(), tables, 8 * cells, hipMemcpyDeviceToHost, st));
    PH_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0.f;
    PH_HIP_CHECK(hipEventElapsedTime(&ms, lane.lane->ev_start, lane.lane->ev_stop));
    dev_ms += (double)ms;
    stats.scan_kernel = PH_KERNEL_SCAN_FILTERED;
  } else {
    // nothing to scan: every cell keeps its identity
    for (int s = 0; s < ns; ++s) {
      const int op = fp.slot_op[s];
      const long long idv = (op == FOP_MIN_I || op == FOP_MIN_F) ? INT64_MAX
                            : ((op == FOP_MAX_I || op == FOP_MAX_F) ? INT64_MIN : 0);
      std::fill(host_tables.begin() + (ptrdiff_t)(cnt_cells + pc_cells + (size_t)s * (size_t)G),
                host_tables.begin() + (ptrdiff_t)(cnt_cells + pc_cells + (size_t)(s + 1) * (size_t)G), idv);
    }
    stats.scan_kernel = PH_KERNEL_SCAN_FILTERED;
  }
  const unsigned long long* seg_count = reinterpret_cast<const unsigned long long*>(host_tables.data());
  const unsigned long long* pcount = reinterpret_cast<const unsigned long long*>(host_tables.data() + cnt_cells);
  const long long* slot_tab = host_tables.data() + cnt_cells + pc_cells;

  // ---- statistics: the sums over each segment's pipelines (FilteredAggregationOperator.java:89-91,
  // FilteredGroupByOperator.java:149-151)
  std::vector<int64_t> seg_of(nseg, -1);
  for (size_t d = 0; d < nfs; ++d) seg_of[(size_t)fseg_src[d]] = (int64_t)d;
  for (int i = 0; i < nseg; ++i) {
    if (main_cls[i] == FP_EMPTY) continue;  // one pipeline over the empty main filter: no docs, no entries
    const int64_t nd = segs[i]->num_docs;
    const int64_t main_docs = main_cls[i] == FP_ALL ? nd : main_bm[i].docs;
    auto pipe_docs = [&](int p) {
      return seg_of[(size_t)i] < 0 ? (int64_t)0 : (int64_t)seg_count[(size_t)seg_of[(size_t)i] * kFMaxPipes + (size_t)p];
    };
    std::vector<char> unf((size_t)P, 0);  // the pipelines whose functions run in the unfiltered pipeline
    unf[0] = has_unfiltered;
    for (int f = 0; f < K; ++f) {
      const int32_t c = sub_cls[i][f];
      std::vector<char> own((size_t)P, 0);
      own[(size_t)f + 1] = 1;
      int64_t docs = 0, entries = 0;
      if (main_cls[i] == FP_ALL) {
        // the sub-filter stands alone (:219-220): its own operator, its ordinary statistic
        docs = c == FP_EMPTY ? 0 : (c == FP_ALL ? nd : sub_bm[i][f].docs);
        entries = c >= FP_SCAN_LEAF ? sub_bm[i][f].entries : 0;
      } else if (c == FP_EMPTY) {
        docs = 0;  // (:222-223) the empty operator
      } else if (c == FP_ALL) {
        unf[(size_t)f + 1] = 1;  // (:224-225, :243-245)
        continue;
      } else {
        // CombinedFilterOperator (CombinedFilterOperator.java:62-67): AndDocIdSet over [bitmap of main, sub].  The main
        // doc set is materialised by toNonScanDocIdSet, whose scan is not counted (BlockDocIdSet.java:54-68); a scan
        // leaf is then applied to main's docs (one entry each), an index leaf scans nothing
        docs = pipe_docs(f + 1);
        entries = c == FP_SCAN_LEAF ? main_docs : 0;
      }
      stats.num_docs_scanned += docs;
      stats.num_entries_scanned_in_filter += entries;
      stats.num_entries_scanned_post_filter += docs * projected(own);
    }
    bool any_unf = false;
    for (int p = 0; p < P; ++p) any_unf = any_unf || unf[(size_t)p];
    bool unf_has_fn = false;
    for (int k = 0; k < nagg; ++k) unf_has_fn = unf_has_fn || unf[(size_t)agg_pipe[k]];
    if (any_unf && unf_has_fn) {
      stats.num_docs_scanned += main_docs;
      stats.num_entries_scanned_in_filter += main_cls[i] == FP_ALL ? 0 : main_bm[i].entries;
      stats.num_entries_scanned_post_filter += main_docs * projected(unf);
    }
  }

  // ---- result rows
  res->agg_types.resize((size_t)nagg);
  res->agg_log2m.assign((size_t)nagg, 0);
  for (int k = 0; k < nagg; ++k) res->agg_types[(size_t)k] = q->aggregations[k].type;
  // the docs pipeline p saw of row g, and the value of aggregation k there; an empty cell holds the result holder's
  // default: COUNT 0 (CountAggregationFunction.java:38 DEFAULT_INITIAL_VALUE), SUM 0.0 (SumAggregationFunction.java:38
  // DEFAULT_VALUE), MIN +Infinity (MinAggregationFunction.java:38), MAX -Infinity (MaxAggregationFunction.java:38)
  auto cell = [&](int k, int64_t g, int64_t docs) -> double {
    const int t = q->aggregations[k].type;
    const long long raw = slot_tab[(size_t)agg_slot[k] * (size_t)G + (size_t)g];
    const int op = fp.slot_op[agg_slot[k]];
    double v;
    if (t == PH_AGG_SUM) {
      if (op == FOP_SUM_I) {
        v = (double)raw;
        if (raw >= (int64_t(1) << 53) || raw <= -(int64_t(1) << 53)) stats.sum_precision_flag = 1;
      } else {
        memcpy(&v, &raw, 8);
        if (op == FOP_SUM_I2F && std::fabs(v) >= 9007199254740992.0) stats.sum_precision_flag = 1;
      }
    } else if (docs == 0) {
      v = t == PH_AGG_MIN ? INFINITY : -INFINITY;
    } else {
      v = (op == FOP_MIN_I || op == FOP_MAX_I) ? (double)raw : double_from_order_key(raw);
    }
    return v;
  };
  res->aggs.resize((size_t)nagg);
  if (group_cols.empty()) {
    std::vector<int64_t> docs((size_t)P, 0);
    for (size_t d = 0; d < nfs; ++d)
      for (int p = 0; p < P; ++p) docs[(size_t)p] += (int64_t)seg_count[d * kFMaxPipes + (size_t)p];
    for (int k = 0; k < nagg; ++k) {
      res->aggs[(size_t)k].assign(8, 0);
      const int64_t n = docs[(size_t)agg_pipe[k]];
      if (q->aggregations[k].type == PH_AGG_COUNT) {
        memcpy(res->aggs[(size_t)k].data(), &n, 8);
      } else {
        const double v = cell(k, 0, n);
        memcpy(res->aggs[(size_t)k].data(), &v, 8);
      }
    }
    res->num_groups = 1;
  } else {
    std::vector<int64_t> rows;
    for (int64_t g = 0; g < G && pc_cells; ++g) {
      bool any = false;
      for (int p = 0; p < P && !any; ++p) any = pcount[(size_t)p * (size_t)G + (size_t)g] != 0;
      if (any) rows.push_back(g);
    }
    const size_t R = rows.size();
    res->keys.resize(group_cols.size());
    for (size_t c = 0; c < group_cols.size(); ++c) {
      const Dictionary& d = gdicts[c]->dict;
      const int32_t es = entry_size_of(d);
      res->key_types.push_back(d.type);
      res->key_entry_size.push_back(es);
      res->keys[c].assign(R * (size_t)es, 0);
      const int64_t sz = std::max<int64_t>(1, d.size);
      for (size_t r = 0; r < R; ++r)
        put_key(d, (rows[r] / fp.group_stride[c]) % sz, res->keys[c].data() + r * (size_t)es, es);
    }
    for (int k = 0; k < nagg; ++k) {
      res->aggs[(size_t)k].assign(8 * R, 0);
      for (size_t r = 0; r < R; ++r) {
        const int64_t n = (int64_t)pcount[(size_t)agg_pipe[k] * (size_t)G + (size_t)rows[r]];
        if (q->aggregations[k].type == PH_AGG_COUNT) {
          memcpy(res->aggs[(size_t)k].data() + 8 * r, &n, 8);
        } else {
          const double v = cell(k, rows[r], n);
          memcpy(res->aggs[(size_t)k].data() + 8 * r, &v, 8);
        }
      }
    }
    res->num_groups = (int64_t)R;
  }
  const int plan_mode = mode == MODE_AGG ? 1 : (mode == MODE_GROUP_LDS ? 2 : 3);
  res->mode = plan_mode;
  stats.plan_mode = plan_mode;
  stats.num_devices = 1;
  stats.device_ms = dev_ms;
  stats.host_ms = std::max(0.0, std::chrono::duration<double, std::milli>(clock::now() - t0).count() - dev_ms);
  return res.release();
}

}  // namespace ph
