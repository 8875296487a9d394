// bquery_parser.hpp -- the boolean layer of femto's query language: AND OR NOT THEN WITHIN over regular-expression leaves.
//
// The reference's grammar (src/main/posix.bison.y:122-135) puts two productions above regexp_top:
//     boolean_exp  := boolean_exp boolean_op boolean_rest | boolean_rest           left-associative, no precedence
//     boolean_rest := regexp_top | '(' boolean_exp boolean_op boolean_rest ')'
// flex and bison are not available to this build, so -- as ../csrc/query_parser.hpp does for the layers below -- the rules are
// restated by hand.  The tokens are query_parser.hpp's own (QueryLexer; that file is included, not edited):
//   * QTok::BOOL carries the keyword and its byte offset.  The lexer drops WITHIN's distance and ends THEN at the keyword, so the
//     number is read again from the text here (read_int_part, posix.flex.l:101-106: sscanf "%i", default INT_MAX):
//     THEN takes [[:space:]]+[[:digit:]]* only when whitespace follows the digits (posix.flex.l:279: flex takes the longest
//     match, the bare keyword is the other alternative), so "a then 20 b" is THEN 20 and "a then 20b" is THEN INT_MAX with the
//     leaf "20b"; the tokens the lexer made of consumed digits are dropped.
//   * A '(' whose content holds a BOOL token at its own depth opens a boolean group; it takes no repeat operator and nothing
//     may stand next to it but an operator, a ')' or the end.  Every other '(' belongs to a regular expression, and a BOOL token
//     inside it is a syntax error.
//   * A leaf is the run of tokens up to the next operator at its depth, the ')' of the enclosing boolean group or the end; it is
//     regexp_top, so APPROX may lead it.  The leaf is handed on as a SLICE OF THE TEXT: the caller compiles it with
//     femto_amd_query_compile, which is the whole pipeline of a query without operators (QueryParser, streamline_query -- the
//     reference streamlines into boolean nodes, query_planning.c:33 -- simplify_query, icase_ast).  The lexer looks one character
//     past a word, so a slice that ended at a ')' gets a '#' (punctuation too, and the start of a comment) appended; bq_parse
//     checks that every slice lexes to exactly the tokens it had in context.
// TYPES (setup_generic_boolean_query, src/main/server.c:5369; results.c:513-545, 763-773): AND OR NOT ask their leaves for
// documents, THEN WITHIN for (document, offset) pairs; AND and NOT take either kind and yield documents; OR needs equal kinds and
// yields that kind; THEN and WITHIN need pairs on both sides.  A tree the reference would fail with ERR_PARAM while it runs is
// refused here, by operator and byte offset.  Limit: 4095 nodes per tree.
#pragma once
#include <algorithm>
#include <cerrno>
#include <climits>
#include <cstdint>
#include <string>
#include <vector>

#include "../csrc/query_parser.hpp"

namespace femto_amd {

enum BqOp { BQ_LEAF = 0, BQ_AND = 1, BQ_OR = 2, BQ_NOT = 3, BQ_THEN = 4, BQ_WITHIN = 5 };   // FEMTO_AMD_BQUERY_* (femto_amd.h)
enum BqType { BQ_DOCUMENTS = 0, BQ_PAIRS = 1 };
constexpr int kBqMaxNodes = 4095;     // per tree (2048 leaves): a chain is as deep as it is long, and a level is a launch

struct BqNode {
  int op = BQ_LEAF;
  int distance = 0;          // THEN / WITHIN
  int left = -1, right = -1; // nodes (postfix order: both stand before this one)
  int leaf = -1;             // BQ_LEAF: index into BqTree::leaves
  int type = BQ_DOCUMENTS;
  int height = 0;            // leaf 0, operator 1 + max of its children
  int64_t at = 0;            // byte offset of the keyword / of the leaf's first token
};
struct BqTree {
  std::vector<BqNode> nodes;           // postfix; the root is the last one
  std::vector<std::string> leaves;     // the text of each leaf, to be compiled as a query of its own
  std::vector<int64_t> leaf_at;
};

inline const char* bq_op_name(int op) {
  static const char* names[] = {"leaf", "AND", "OR", "NOT", "THEN", "WITHIN"};
  return op >= 0 && op <= BQ_WITHIN ? names[op] : "?";
}

class BqParser {
 public:
  BqParser(const uint8_t* p, int64_t n) : p_(p), n_(n) {}
  // false: *err is set; *type_error tells a tree that parses but does not type
  bool parse(BqTree* out, std::string* err, bool* type_error) {
    *type_error = false;
    if (n_ > kRegexMaxLen) { *err = "pattern text too long"; return false; }
    std::vector<QTok> toks;
    QueryLexer lx(p_, n_);
    if (!lx.run(&toks, err)) return false;
    if (!distances(toks, err)) return false;
    if (!trailing_keyword(err)) return false;
    out_ = out;
    int root = -1;
    if (!exp(&root)) { *err = err_; return false; }
    if (cur().kind != QTok::END) { *err = "syntax error at byte " + std::to_string(cur().at); return false; }
    // a query that is one leaf yields its document list
    if (!type_of(root, BQ_DOCUMENTS)) { *err = err_; *type_error = true; return false; }
    return true;
  }

 private:
  const uint8_t* p_;
  int64_t n_;
  std::vector<QTok> t_;
  std::vector<int> dist_;      // per token of t_: the distance of a BOOL token
  size_t k_ = 0;
  int depth_ = 0;
  BqTree* out_ = nullptr;
  std::string err_;

  const QTok& cur() const { return t_[k_]; }
  bool fail(const std::string& m) { err_ = m + " at byte " + std::to_string(cur().at); return false; }
  bool space_at(int64_t k) const { return k < n_ && q_is_space(p_[k]); }
  static bool same(const QTok& a, const QTok& b) {
    if (a.kind != b.kind || a.ch != b.ch || a.str != b.str || a.rmin != b.rmin || a.rmax != b.rmax) return false;
    for (int i = 0; i < 4; i++) if (a.approx[i] != b.approx[i]) return false;
    return true;
  }
  // read_int_part on digits [d, e): sscanf "%i" (a leading 0 is octal)
  bool number(int64_t d, int64_t e, int64_t at, int* out, std::string* err) const {
    const std::string s(reinterpret_cast<const char*>(p_ + d), size_t(e - d));
    errno = 0;
    const long long v = strtoll(s.c_str(), nullptr, 0);
    if (errno || v > INT_MAX) { *err = "distance too large at byte " + std::to_string(at); return false; }
    *out = int(v);
    return true;
  }
  // the distances of THEN and WITHIN, re-read from the text; t_ = the tokens without those THEN's digits made
  bool distances(const std::vector<QTok>& toks, std::string* err) {
    int64_t skip_from = 0, skip_to = 0;
    for (const QTok& t : toks) {
      if (t.kind != QTok::END && t.at >= skip_from && t.at < skip_to) continue;
      int d = 0;
      if (t.kind == QTok::BOOL) {
        const int len = int(std::string(t.word).size());
        const bool then = len == 4 && t.word[0] == 'T', within = len == 6;
        if (then || within) {
          int64_t j = t.at + len;
          while (space_at(j)) j++;
          const int64_t d0 = j;
          while (j < n_ && q_is_digit(p_[j])) j++;
          d = INT_MAX;
          if (j > d0 && space_at(j)) {
            if (!number(d0, j, t.at, &d, err)) return false;
            skip_from = d0;
            skip_to = j;
          }
        }
      }
      t_.push_back(t);
      dist_.push_back(d);
    }
    return true;
  }
  // STRICTER THAN THE REFERENCE: its scanner knows a keyword by the whitespace behind it, so a keyword that ENDS the text is
  // letters to it and "a AND" searches for the string "aAND".  Nobody means that; an operator without a right side is refused.
  bool trailing_keyword(std::string* err) const {
    static const char* words[] = {"AND", "and", "OR", "or", "NOT", "not", "THEN", "then"};
    for (const char* w : words) {
      const int64_t len = int64_t(std::string(w).size()), at = n_ - len;
      if (at < 0 || std::string(reinterpret_cast<const char*>(p_ + at), size_t(len)) != w) continue;
      if (at > 0 && !q_is_space(p_[at - 1])) continue;
      for (const QTok& t : t_)                  // a token starts there: the word stands in no quote, set or comment
        if (t.kind != QTok::END && t.at == at && (t.kind == QTok::STRING || t.kind == QTok::CHARACTER)) {
          *err = std::string("syntax error: ") + w + " at byte " + std::to_string(at) + " has no right side";
          return false;
        }
    }
    return true;
  }
  static int op_of(const QTok& t) {
    switch (t.word[0]) {
      case 'A': return BQ_AND;
      case 'O': return BQ_OR;
      case 'N': return BQ_NOT;
      case 'T': return BQ_THEN;
      default: return BQ_WITHIN;
    }
  }
  int push(const BqNode& n) {
    out_->nodes.push_back(n);
    return int(out_->nodes.size()) - 1;
  }
  // boolean_exp
  bool exp(int* node) {
    int left = -1;
    if (!rest(&left)) return false;
    while (cur().kind == QTok::BOOL) {
      if (out_->nodes.size() + 2 > size_t(kBqMaxNodes)) return fail("too many operators in one query");
      BqNode n;
      n.op = op_of(cur());
      n.distance = dist_[k_];
      n.at = cur().at;
      k_++;
      int right = -1;
      if (!rest(&right)) return false;
      n.left = left;
      n.right = right;
      n.height = 1 + std::max(out_->nodes[size_t(left)].height, out_->nodes[size_t(right)].height);
      left = push(n);
    }
    *node = left;
    return true;
  }
  // does the group opened by token `open` hold a BOOL token at its own depth?  *close = its ')' (or the END token)
  bool boolean_group(size_t open, size_t* close) const {
    int depth = 0;
    bool has = false;
    size_t k = open;
    for (; t_[k].kind != QTok::END; k++) {
      if (t_[k].kind == QTok::GROUP_START) depth++;
      else if (t_[k].kind == QTok::GROUP_END && --depth == 0) break;
      else if (t_[k].kind == QTok::BOOL && depth == 1) has = true;
    }
    *close = k;
    return has;
  }
  // boolean_rest
  bool rest(int* node) {
    size_t close = 0;
    if (cur().kind == QTok::GROUP_START && boolean_group(k_, &close)) {
      if (t_[close].kind != QTok::GROUP_END) { k_ = close; return fail("missing )"); }
      k_++;
      if (++depth_ > kRegexMaxDepth) return fail("parentheses nested too deeply");
      const bool ok = exp(node);
      depth_--;
      if (!ok) return false;
      if (k_ != close) return fail("syntax error");
      k_++;
      if (cur().kind != QTok::BOOL && cur().kind != QTok::GROUP_END && cur().kind != QTok::END)
        return fail("syntax error: a boolean group takes no repeat operator and joins nothing");
      return true;
    }
    return leaf(node);
  }
  // regexp_top, as a slice of the text
  bool leaf(int* node) {
    const size_t first = k_;
    int depth = 0;
    for (;; k_++) {
      const QTok::Kind kd = cur().kind;
      if (kd == QTok::END) break;
      if (kd == QTok::GROUP_START) depth++;
      else if (kd == QTok::GROUP_END) { if (depth == 0) break; depth--; }
      else if (kd == QTok::BOOL) {
        if (depth == 0) break;
        return fail(std::string("syntax error: ") + cur().word + " inside the parentheses of a regular expression");
      }
    }
    if (k_ == first) return fail(cur().kind == QTok::END ? "pattern ends where a term was expected" : "syntax error");
    const int64_t b = t_[first].at, e = cur().at;
    std::string text(reinterpret_cast<const char*>(p_ + b), size_t(e - b));
    if (cur().kind == QTok::GROUP_END) text.push_back('#');
    {                                  // the slice on its own lexes to the tokens it had in context
      std::vector<QTok> alone;
      std::string lerr;
      QueryLexer lx(reinterpret_cast<const uint8_t*>(text.data()), int64_t(text.size()));
      bool ok = lx.run(&alone, &lerr) && alone.size() == k_ - first + 1;
      for (size_t i = 0; ok && i + 1 < alone.size(); i++) ok = same(alone[i], t_[first + i]);
      if (!ok) { k_ = first; return fail("syntax error: this term cannot be read on its own"); }
    }
    BqNode n;
    n.leaf = int(out_->leaves.size());
    n.at = b;
    out_->leaves.push_back(std::move(text));
    out_->leaf_at.push_back(b);
    *node = push(n);
    return true;
  }
  // sets the types below node i; `wanted` is what the parent asks a leaf for
  bool type_of(int i, int wanted) {
    BqNode& n = out_->nodes[size_t(i)];
    if (n.op == BQ_LEAF) { n.type = wanted; return true; }
    const int ask = n.op == BQ_THEN || n.op == BQ_WITHIN ? BQ_PAIRS : BQ_DOCUMENTS;
    if (!type_of(n.left, ask) || !type_of(n.right, ask)) return false;
    const int lt = out_->nodes[size_t(n.left)].type, rt = out_->nodes[size_t(n.right)].type;
    auto name = [](int t) { return t == BQ_PAIRS ? "(document, offset) pairs" : "documents"; };
    if (n.op == BQ_AND || n.op == BQ_NOT) { n.type = BQ_DOCUMENTS; return true; }
    if (n.op == BQ_OR) {
      if (lt != rt) {
        err_ = std::string("type error: OR at byte ") + std::to_string(n.at) + " joins " + name(lt) + " with " + name(rt);
        return false;
      }
      n.type = lt;
      return true;
    }
    if (lt != BQ_PAIRS || rt != BQ_PAIRS) {
      err_ = std::string("type error: ") + bq_op_name(n.op) + " at byte " + std::to_string(n.at) + " needs (document, offset) pairs on both sides; its " +
             (lt != BQ_PAIRS ? "left" : "right") + " side yields documents";
      return false;
    }
    n.type = BQ_PAIRS;
    return true;
  }
};

// the tree printed back as ast_to_string prints AST_NODE_BOOL (src/main/ast.c:1078-1110): left, " OP " (THEN and WITHIN with
// "%i" of the distance), right -- no parentheses; leaf_echo(l) is the leaf's own echo
template <class F>
inline void bq_echo(const BqTree& t, int i, F leaf_echo, std::string& o) {
  const BqNode& n = t.nodes[size_t(i)];
  if (n.op == BQ_LEAF) { o += leaf_echo(n.leaf); return; }
  bq_echo(t, n.left, leaf_echo, o);
  o += " ";
  o += bq_op_name(n.op);
  if (n.op == BQ_THEN || n.op == BQ_WITHIN) o += " " + std::to_string(n.distance);
  o += " ";
  bq_echo(t, n.right, leaf_echo, o);
}

}  // namespace femto_amd
