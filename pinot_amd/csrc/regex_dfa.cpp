// regex_dfa.cpp -- regex_compile: a REGEXP_LIKE pattern (the java.util.regex subset of DESIGN.md, compiled as the
// reference does with CASE_INSENSITIVE | UNICODE_CASE) to the byte-level DFA k_regex_dict walks (regex_dfa.h).
//
//   pattern --parse--> syntax tree over code-point sets --emit--> byte-level NFA (UTF-8 paths) --subsets--> DFA
//
// Every code-point set the subset can name is an ASCII bitmap, some of seven special non-ASCII code points (the three
// non-ASCII line terminators and the four code points that case-fold to an ASCII letter) and "every other non-ASCII
// code point" in or out, so no Unicode table is needed.  Host code only; it depends on nothing but the two headers.
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "pinot_hip.h"
#include "regex_dfa.h"

namespace ph {

[[noreturn]] void fail(int code, const std::string& msg);
RegexProgram regex_compile(const std::string& pattern);

namespace {

// U+0085 U+2028 U+2029 (line terminators), U+017F (folds to s), U+212A (to k), U+0130 and U+0131 (to i)
constexpr uint32_t kSpecial[7] = {0x85, 0x2028, 0x2029, 0x17F, 0x212A, 0x130, 0x131};

struct CpSet {
  uint64_t ascii[2] = {0, 0};
  uint8_t special = 0;  // bit k: kSpecial[k]
  bool other = false;   // every non-ASCII code point that is not special
  void add(uint32_t c) { ascii[c >> 6] |= 1ull << (c & 63); }
  bool has(uint32_t c) const { return (ascii[c >> 6] >> (c & 63)) & 1u; }
  bool holds(uint32_t cp) const {  // any code point
    if (cp < 128) return has(cp);
    for (int k = 0; k < 7; ++k)
      if (cp == kSpecial[k]) return (special >> k) & 1u;
    return other;
  }
  void unite(const CpSet& o) {
    ascii[0] |= o.ascii[0];
    ascii[1] |= o.ascii[1];
    special |= o.special;
    other = other || o.other;
  }
  CpSet complement() const {
    CpSet r;
    r.ascii[0] = ~ascii[0];
    r.ascii[1] = ~ascii[1];
    r.special = (uint8_t)(~special & 0x7F);
    r.other = !other;
    return r;
  }
};

uint32_t upper(uint32_t c) { return c >= 'a' && c <= 'z' ? c - 32 : c; }
uint32_t lower(uint32_t c) { return c >= 'A' && c <= 'Z' ? c + 32 : c; }

// CASE_INSENSITIVE | UNICODE_CASE over ASCII members: a code point ch matches when ch, upper(ch) or lower(upper(ch))
// is a member (java.util.regex's CIRangeU; a single character is folded to both cases before, as SingleU does)
CpSet fold_case(const CpSet& f) {
  CpSet r;
  for (uint32_t c = 0; c < 128; ++c)
    if (f.has(c) || f.has(upper(c)) || f.has(lower(upper(c)))) r.add(c);
  if (f.has('S') || f.has('s')) r.special |= 1u << 3;  // upper(U+017F) = S
  if (f.has('k')) r.special |= 1u << 4;                // U+212A is its own upper case; its lower case is k
  if (f.has('i')) r.special |= 1u << 5;                // U+0130 likewise, to i
  if (f.has('I') || f.has('i')) r.special |= 1u << 6;  // upper(U+0131) = I
  return r;
}

CpSet predefined(char k) {  // \d \w \s and their complements: ASCII-defined, never case folded
  CpSet s;
  const char l = (char)lower((uint32_t)k);
  if (l == 'd' || l == 'w')
    for (uint32_t c = '0'; c <= '9'; ++c) s.add(c);
  if (l == 'w') {
    for (uint32_t c = 'a'; c <= 'z'; ++c) { s.add(c); s.add(c - 32); }
    s.add('_');
  }
  if (l == 's')
    for (char c : {' ', '\t', '\n', '\v', '\f', '\r'}) s.add((uint32_t)c);
  return k == l ? s : s.complement();
}

CpSet dot_set() {  // one code point that is no line terminator
  CpSet s;
  s.add('\n');
  s.add('\r');
  s.special = 0x07;
  return s.complement();
}

[[noreturn]] void unsupported(const std::string& what) { fail(PH_ERR_UNSUPPORTED, "REGEXP_LIKE: " + what); }
[[noreturn]] void bad(const std::string& what) { fail(PH_ERR_BAD_QUERY, "REGEXP_LIKE: " + what); }

// ------------------------------------------------------------------------------------------------- syntax tree
enum AstKind { A_EMPTY, A_SET, A_CAT, A_ALT, A_REP, A_BOL, A_EOL };
constexpr int kInf = -1;

struct Ast {
  AstKind kind = A_EMPTY;
  CpSet set;
  int min = 0, max = 0;  // A_REP; max == kInf: unbounded
  std::vector<int> kids;
};

struct Parser {
  const std::string& p;
  size_t i = 0;
  int depth = 0;
  std::vector<Ast> ast;

  explicit Parser(const std::string& pattern) : p(pattern) {
    for (unsigned char c : p) {
      if (c >= 0x80) unsupported("a non-ASCII character in the pattern");
      if (c == '\n' || c == '\r') unsupported("a line terminator in the pattern");
    }
  }
  bool more() const { return i < p.size(); }
  char peek() const { return p[i]; }
  int node(AstKind k) {
    ast.emplace_back();
    ast.back().kind = k;
    return (int)ast.size() - 1;
  }
  int set_node(const CpSet& s) {
    const int n = node(A_SET);
    ast[(size_t)n].set = s;
    return n;
  }
  int literal(uint32_t c) {
    CpSet f;
    f.add(lower(c));
    f.add(upper(c));
    return set_node(fold_case(f));
  }

  // \x after the backslash, outside and inside a class: the refusals, each with its own message
  [[noreturn]] void refuse_escape(char c) {
    if (c >= '1' && c <= '9') unsupported("a backreference (\\" + std::string(1, c) + ")");
    if (c == 'k') unsupported("a named backreference (\\k)");
    if (strchr("bBAzZG", c)) unsupported("the boundary matcher \\" + std::string(1, c));
    if (c == 'p' || c == 'P') unsupported("a \\p{} property or POSIX class");
    if (c == 'Q' || c == 'E') unsupported("a \\Q..\\E quotation");
    if (strchr("ux0c", c)) unsupported("a \\" + std::string(1, c) + " character escape");
    unsupported("the escape \\" + std::string(1, c));
  }
  // a backslash escape that names one character: its code, or -1
  static int escaped_char(char c) {
    switch (c) {
      case 't': return '\t';
      case 'n': return '\n';
      case 'r': return '\r';
      case 'f': return '\f';
      case 'a': return 0x07;
      case 'e': return 0x1B;
      default: break;
    }
    const bool alnum = (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z');
    return alnum ? -1 : (unsigned char)c;
  }

  int parse() {
    const int r = alternation();
    if (more()) bad("unmatched closing parenthesis");  // alternation stops only at `)` or the end
    return r;
  }
  int alternation() {
    std::vector<int> alts{sequence()};
    while (more() && peek() == '|') {
      ++i;
      alts.push_back(sequence());
    }
    if (alts.size() == 1) return alts[0];
    const int n = node(A_ALT);
    ast[(size_t)n].kids = alts;
    return n;
  }
  int sequence() {
    std::vector<int> items;
    while (more() && peek() != '|' && peek() != ')') items.push_back(quantified());
    if (items.empty()) return node(A_EMPTY);
    if (items.size() == 1) return items[0];
    const int n = node(A_CAT);
    ast[(size_t)n].kids = items;
    return n;
  }
  int quantified() {
    int a = atom();
    if (!more()) return a;
    int mn, mx;
    const char c = peek();
    if (c == '*') { mn = 0; mx = kInf; ++i; }
    else if (c == '+') { mn = 1; mx = kInf; ++i; }
    else if (c == '?') { mn = 0; mx = 1; ++i; }
    else if (c == '{') { ++i; counts(&mn, &mx); }
    else return a;
    if (more() && peek() == '?') ++i;  // lazy: the same language for a yes/no find()
    else if (more() && peek() == '+') unsupported("a possessive quantifier");
    if (more() && (peek() == '*' || peek() == '+' || peek() == '?'))
      bad("dangling quantifier " + std::string(1, peek()));
    const int n = node(A_REP);
    ast[(size_t)n].min = mn;
    ast[(size_t)n].max = mx;
    ast[(size_t)n].kids = {a};
    return n;
  }
  int number() {
    if (!more() || peek() < '0' || peek() > '9') bad("illegal repetition");
    int v = 0;
    while (more() && peek() >= '0' && peek() <= '9') {
      v = v * 10 + (peek() - '0');
      if (v > kRegexMaxNfa)
        unsupported("the pattern needs more than " + std::to_string(kRegexMaxNfa) + " NFA nodes (a repetition count)");
      ++i;
    }
    return v;
  }
  void counts(int* mn, int* mx) {  // after `{`
    *mn = *mx = number();
    if (more() && peek() == ',') {
      ++i;
      *mx = (more() && peek() == '}') ? kInf : number();
    }
    if (!more() || peek() != '}') bad("unclosed counted repetition");
    ++i;
    if (*mx != kInf && *mx < *mn) bad("illegal repetition range");
  }
  int atom() {
    const char c = p[i++];
    switch (c) {
      case '(': return group();
      case '[': return char_class();
      case '.': return set_node(dot_set());
      case '^': return node(A_BOL);
      case '$': return node(A_EOL);
      case '*': case '+': case '?': bad("dangling quantifier " + std::string(1, c));
      // java.util.regex reads this as a repetition of nothing; its meaning is not restated here
      case '{': unsupported("a counted repetition that follows a quantifier or nothing");
      case '\\': {
        if (!more()) bad("a trailing backslash");
        const char e = p[i++];
        if (strchr("dwsDWS", e)) return set_node(predefined(e));
        const int ch = escaped_char(e);
        if (ch < 0) refuse_escape(e);
        return literal((uint32_t)ch);
      }
      default: return literal((unsigned char)c);
    }
  }
  int group() {
    if (more() && peek() == '?') {
      ++i;
      if (!more()) bad("unclosed group");
      const char k = p[i++];
      if (k == '=' || k == '!') unsupported("lookahead");
      if (k == '<') {
        if (more() && (peek() == '=' || peek() == '!')) unsupported("lookbehind");
        unsupported("a named group");
      }
      if (k == '>') unsupported("an atomic group");
      if (k != ':') unsupported("inline flags");
    }
    if (++depth > 200) unsupported("groups nested deeper than 200");
    const int r = alternation();
    --depth;
    if (!more()) bad("unclosed group");
    ++i;  // `)`
    return r;
  }
  int char_class() {
    bool negate = false;
    if (more() && peek() == '^') { negate = true; ++i; }
    CpSet folded, plain;  // literals and ranges (case folded at the end); predefined classes (never folded)
    bool first = true;
    for (;; first = false) {
      if (!more()) bad("unclosed character class");
      char c = p[i++];
      if (c == ']' && !first) break;
      if (c == '[') unsupported("a nested character class");
      if (c == '&' && more() && peek() == '&') unsupported("a character class intersection (&&)");
      int lo = (unsigned char)c;
      if (c == '\\') {
        if (!more()) bad("a trailing backslash");
        const char e = p[i++];
        if (strchr("dwsDWS", e)) {
          plain.unite(predefined(e));
          if (i + 1 < p.size() && peek() == '-' && p[i + 1] != ']') unsupported("a range from a predefined class");
          continue;
        }
        lo = escaped_char(e);
        if (lo < 0) refuse_escape(e);
      }
      if (i + 1 < p.size() && peek() == '-' && p[i + 1] != ']') {  // a range
        ++i;
        char h = p[i++];
        int hi = (unsigned char)h;
        if (h == '[') unsupported("a nested character class");
        if (h == '\\') {
          if (!more()) bad("a trailing backslash");
          const char e = p[i++];
          if (strchr("dwsDWS", e)) unsupported("a range to a predefined class");
          hi = escaped_char(e);
          if (hi < 0) refuse_escape(e);
        }
        if (hi < lo) bad("illegal character range");
        for (int x = lo; x <= hi; ++x) folded.add((uint32_t)x);
      } else {
        folded.add(lower((uint32_t)lo));
        folded.add(upper((uint32_t)lo));
      }
    }
    CpSet s = fold_case(folded);
    s.unite(plain);
    return set_node(negate ? s.complement() : s);
  }
};

// ------------------------------------------------------------------------------------------------- byte-level NFA
enum NodeKind : uint8_t { N_BYTES, N_SPLIT, N_BOL, N_EOL, N_ACCEPT };

struct Bytes {
  uint64_t w[4] = {0, 0, 0, 0};
  void add(uint32_t b) { w[b >> 6] |= 1ull << (b & 63); }
  bool has(uint32_t b) const { return (w[b >> 6] >> (b & 63)) & 1u; }
  bool any() const { return w[0] | w[1] | w[2] | w[3]; }
  bool operator<(const Bytes& o) const { return std::lexicographical_compare(w, w + 4, o.w, o.w + 4); }
};

struct Node {
  NodeKind kind;
  int out = -1, out1 = -1;  // N_SPLIT: two epsilons (out1 may be -1); the others: out
  Bytes bytes;              // N_BYTES: the bytes that lead to out
};

struct Nfa {
  std::vector<Node> nodes;
  const std::vector<Ast>& ast;
  int emits = 0;
  explicit Nfa(const std::vector<Ast>& a) : ast(a) {}

  int add(NodeKind k, int out, int out1 = -1) {
    if ((int)nodes.size() >= kRegexMaxNfa)
      unsupported("the pattern needs more than " + std::to_string(kRegexMaxNfa) + " NFA nodes");
    Node n;
    n.kind = k;
    n.out = out;
    n.out1 = out1;
    nodes.push_back(n);
    return (int)nodes.size() - 1;
  }

  // the UTF-8 byte paths of a code-point set, all ending in `next`: its entry node, or -1 for the empty set.  Nodes
  // with the same bytes and target are shared between the paths.
  int emit_set(const CpSet& s, int next) {
    std::map<std::pair<Bytes, int>, int> memo;
    auto step = [&](const Bytes& b, int out) {
      auto key = std::make_pair(b, out);
      auto it = memo.find(key);
      if (it != memo.end()) return it->second;
      const int n = add(N_BYTES, out);
      nodes[(size_t)n].bytes = b;
      memo.emplace(key, n);
      return n;
    };
    auto cont_bytes = [](uint64_t mask) {  // continuation bytes 0x80 + bit
      Bytes b;
      b.w[2] = mask;
      return b;
    };
    std::vector<int> entries;
    Bytes one;
    one.w[0] = s.ascii[0];
    one.w[1] = s.ascii[1];
    if (one.any()) entries.push_back(step(one, next));
    // two bytes: lead C2..DF, the continuation mask per lead; leads with the same mask share a path
    std::map<uint64_t, Bytes> two;
    for (uint32_t l = 0xC2; l <= 0xDF; ++l) {
      uint64_t m = 0;
      for (uint32_t c = 0; c < 64; ++c)
        if (s.holds(((l & 0x1Fu) << 6) | c)) m |= 1ull << c;
      if (m) two[m].add(l);
    }
    for (auto& kv : two) entries.push_back(step(kv.second, step(cont_bytes(kv.first), next)));
    // three bytes: lead E0..EF, per (lead, second) the mask of thirds; (leads, seconds) with the same mask share a path
    std::map<uint64_t, std::map<uint32_t, uint64_t>> three;  // third mask -> lead -> seconds mask
    for (uint32_t l = 0xE0; l <= 0xEF; ++l)
      for (uint32_t c2 = 0; c2 < 64; ++c2) {
        uint64_t m = 0;
        for (uint32_t c3 = 0; c3 < 64; ++c3)
          if (s.holds(((l & 0x0Fu) << 12) | (c2 << 6) | c3)) m |= 1ull << c3;
        if (m) three[m][l] |= 1ull << c2;
      }
    for (auto& tm : three) {
      const int third = step(cont_bytes(tm.first), next);
      std::map<uint64_t, Bytes> leads;  // seconds mask -> leads
      for (auto& ls : tm.second) leads[ls.second].add(ls.first);
      for (auto& kv : leads) entries.push_back(step(kv.second, step(cont_bytes(kv.first), third)));
    }
    if (s.other) {  // four bytes: no special code point lies there
      Bytes lead;
      for (uint32_t l = 0xF0; l <= 0xF7; ++l) lead.add(l);
      const uint64_t all = ~0ull;
      entries.push_back(step(lead, step(cont_bytes(all), step(cont_bytes(all), step(cont_bytes(all), next)))));
    }
    if (entries.empty()) return -1;
    int e = entries.back();
    for (size_t k = entries.size() - 1; k-- > 0;) e = add(N_SPLIT, entries[k], e);
    return e;
  }

  // the nodes of syntax-tree node `a`, continuing at `next`: the entry node (-1: nothing can pass)
  int emit(int a, int next) {
    if (++emits > 64 * kRegexMaxNfa)  // repetitions of something empty make no nodes but still take time
      unsupported("the pattern needs more than " + std::to_string(kRegexMaxNfa) + " NFA nodes (nested repetitions)");
    const Ast& t = ast[(size_t)a];
    switch (t.kind) {
      case A_EMPTY: return next;
      case A_SET: return emit_set(t.set, next);
      case A_BOL: return add(N_BOL, next);
      case A_EOL: return add(N_EOL, next);
      case A_CAT: {
        int cur = next;
        for (size_t k = t.kids.size(); k-- > 0 && cur >= 0;) cur = emit(t.kids[k], cur);
        return cur;
      }
      case A_ALT: {
        int e = -1;
        for (size_t k = t.kids.size(); k-- > 0;) {
          const int b = emit(t.kids[k], next);
          if (b < 0) continue;
          e = e < 0 ? b : add(N_SPLIT, b, e);
        }
        return e;
      }
      case A_REP: {
        const int kid = t.kids[0];
        int cur = next, copies = t.min;
        if (t.max == kInf) {
          const int loop = add(N_SPLIT, -1, next);  // once more, or on
          const int body = emit(kid, loop);
          nodes[(size_t)loop].out = body;
          if (t.min == 0) {
            cur = loop;
          } else {  // the last mandatory copy is the loop's body
            cur = body;
            copies = t.min - 1;
          }
        } else {
          for (int k = t.min; k < t.max; ++k) {  // nested optionals
            const int b = emit(kid, cur);
            cur = b < 0 ? next : add(N_SPLIT, b, next);
          }
        }
        for (int k = 0; k < copies && cur >= 0; ++k) cur = emit(kid, cur);
        return cur;
      }
    }
    return -1;
  }
};

// the nodes reachable from `from` through epsilons (and through `^` / `$` edges when allowed) that a DFA state keeps:
// byte nodes, `$` nodes (for a later MARK) and the accept node.  A set that holds the accept node is just that node.
std::vector<int> closure(const Nfa& nfa, const std::vector<int>& from, bool bol, bool eol, int accept) {
  std::vector<char> seen(nfa.nodes.size(), 0);
  std::vector<int> stack, keep;
  auto push = [&](int n) {
    if (n >= 0 && !seen[(size_t)n]) {
      seen[(size_t)n] = 1;
      stack.push_back(n);
    }
  };
  for (int n : from) push(n);
  while (!stack.empty()) {
    const int n = stack.back();
    stack.pop_back();
    const Node& x = nfa.nodes[(size_t)n];
    switch (x.kind) {
      case N_SPLIT: push(x.out); push(x.out1); break;
      case N_BOL: if (bol) push(x.out); break;
      case N_EOL:
        keep.push_back(n);
        if (eol) push(x.out);
        break;
      case N_BYTES: keep.push_back(n); break;
      case N_ACCEPT: return {accept};
    }
  }
  std::sort(keep.begin(), keep.end());
  return keep;
}

}  // namespace

RegexProgram regex_compile(const std::string& pattern) {
  Parser parser(pattern);
  const int root = parser.parse();
  Nfa nfa(parser.ast);
  const int accept = nfa.add(N_ACCEPT, -1);
  const int entry = nfa.emit(root, accept);
  // find() may start at any code point: a restart node that loops on any whole code point, line terminators included
  const int restart = nfa.add(N_SPLIT, -1, entry);
  nfa.nodes[(size_t)restart].out = nfa.emit_set(CpSet().complement(), restart);

  // bytes that lie in the same byte nodes behave alike: provisional classes (the true ones are the table's distinct
  // columns, merged below)
  std::vector<int> cls_of(256), rep;
  {
    std::map<std::vector<int>, int> by_sig;
    for (uint32_t b = 0; b < 256; ++b) {
      std::vector<int> sig;
      for (size_t n = 0; n < nfa.nodes.size(); ++n)
        if (nfa.nodes[n].kind == N_BYTES && nfa.nodes[n].bytes.has(b)) sig.push_back((int)n);
      auto it = by_sig.emplace(sig, (int)rep.size());
      if (it.second) rep.push_back((int)b);
      cls_of[b] = it.first->second;
    }
  }
  const int nprov = (int)rep.size(), mark = nprov;

  // subset construction.  A state is (node set, still at offset 0): only the start state is at offset 0, where MARK
  // (the value is empty, or a lone line terminator follows) lets `^` edges pass as well
  typedef std::pair<std::vector<int>, bool> Key;
  std::map<Key, int> ids;
  std::vector<Key> states;
  std::vector<std::vector<int>> rows;  // [state][provisional class, then MARK]
  auto state_of = [&](std::vector<int> set, bool at0) {
    Key k(std::move(set), at0);
    auto it = ids.find(k);
    if (it != ids.end()) return it->second;
    if ((int)states.size() >= kRegexMaxStates)
      unsupported("the pattern needs more than " + std::to_string(kRegexMaxStates) + " DFA states");
    ids.emplace(k, (int)states.size());
    states.push_back(std::move(k));
    return (int)states.size() - 1;
  };
  const int start = state_of(closure(nfa, {restart}, true, false, accept), true);
  for (size_t s = 0; s < states.size(); ++s) {
    const Key cur = states[s];  // a copy: states grows
    std::vector<int> row((size_t)nprov + 1);
    for (int c = 0; c < nprov; ++c) {
      std::vector<int> moved;
      for (int n : cur.first) {
        const Node& x = nfa.nodes[(size_t)n];
        if (x.kind == N_ACCEPT) moved.push_back(n);  // absorbing
        else if (x.kind == N_BYTES && x.bytes.has((uint32_t)rep[(size_t)c])) moved.push_back(x.out);
      }
      row[(size_t)c] = state_of(closure(nfa, moved, false, false, accept), false);
    }
    row[(size_t)mark] = state_of(closure(nfa, cur.first, cur.second, true, accept), cur.second);
    rows.push_back(std::move(row));
  }

  // the byte classes: the distinct columns of the table
  std::map<std::vector<int>, int> columns;
  std::vector<int> final_of((size_t)nprov), col_rep;
  for (int c = 0; c < nprov; ++c) {
    std::vector<int> col(states.size());
    for (size_t s = 0; s < states.size(); ++s) col[s] = rows[s][(size_t)c];
    auto it = columns.emplace(std::move(col), (int)col_rep.size());
    if (it.second) col_rep.push_back(c);
    final_of[(size_t)c] = it.first->second;
  }
  const int nclasses = (int)col_rep.size() + 1;
  if (nclasses > kRegexMaxClasses)
    unsupported("the pattern needs more than " + std::to_string(kRegexMaxClasses) + " byte classes");

  RegexProgram P{};
  P.h.nstates = (int32_t)states.size();
  P.h.nclasses = nclasses;
  P.h.start = start;
  P.h.mark = nclasses - 1;
  for (uint32_t b = 0; b < 256; ++b) P.h.cls[b] = (uint8_t)final_of[(size_t)cls_of[b]];
  for (size_t s = 0; s < states.size(); ++s) {
    for (size_t k = 0; k < col_rep.size(); ++k)
      P.next[s * (size_t)nclasses + k] = (uint8_t)rows[s][(size_t)col_rep[k]];
    P.next[s * (size_t)nclasses + (size_t)P.h.mark] = (uint8_t)rows[s][(size_t)mark];
    if (states[s].first.size() == 1 && states[s].first[0] == accept) P.h.accept[s >> 5] |= 1u << (s & 31);
  }
  return P;
}

}  // namespace ph
