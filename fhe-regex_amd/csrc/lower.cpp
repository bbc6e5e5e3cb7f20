// Value DAG -> PBS gate program.  See lower.h.
#include "lower.h"

#include <algorithm>
#include <bitset>
#include <map>
#include <queue>
#include <tuple>
#include <cstring>
#include <iterator>
#include <string_view>
#include <unordered_map>

namespace fr {

void lut_eq(uint8_t* lut, int v) {
    for (int x = 0; x < 16; ++x) lut[x] = (uint8_t)(x == v);
}
void lut_sign(uint8_t* lut, int v) {
    for (int x = 0; x < 16; ++x) lut[x] = (uint8_t)(x < v ? 0 : (x == v ? 1 : 2));
}
void lut_gt3(uint8_t* lut, bool le) {
    for (int x = 0; x < 16; ++x) {
        int sh = x / 3, sl = x % 3;
        bool gt = (sh == 2) || (sh == 1 && sl == 2);
        lut[x] = (uint8_t)(le ? !gt : gt);
    }
}
void lut_at_least(uint8_t* lut, int m) {
    for (int x = 0; x < 16; ++x) lut[x] = (uint8_t)(x >= m);
}

PGate nibble_test_gate(bool sign, int pos, int half, int v) {
    PGate g;
    g.ins = {{cblk(pos, 2 * half), 1}, {cblk(pos, 2 * half + 1), 4}};
    if (sign) lut_sign(g.lut, v);
    else lut_eq(g.lut, v);
    return g;
}
PGate cmp_final_gate(VNode::Op op, int lo_gate, int hi_gate) {
    PGate g;
    if (op == VNode::EQ) {
        g.ins = {{lo_gate, 1}, {hi_gate, 1}};
        lut_eq(g.lut, 2);
    } else {
        g.ins = {{hi_gate, 3}, {lo_gate, 1}};
        lut_gt3(g.lut, op == VNode::LE);
    }
    return g;
}
PGate pair_gate(bool is_and, const PairOperand& p, const PairOperand& q) {
    PGate g;
    int offset = 0;
    for (const PairOperand* o : {&p, &q}) {
        if (o->gate < 0) {
            offset += o->c;  // trivial operand (e.g. or(false, x), execution.rs:154-164)
        } else {
            g.ins.push_back({o->gate, o->neg ? -1 : 1});
            offset += o->neg;
        }
    }
    g.offset = 2 * offset;
    if (is_and) lut_eq(g.lut, 2);
    else lut_at_least(g.lut, 1);
    return g;
}

namespace {

struct Lit {
    int gate;
    bool neg;
    bool operator<(const Lit& o) const { return gate != o.gate ? gate < o.gate : neg < o.neg; }
    bool operator==(const Lit& o) const { return gate == o.gate && neg == o.neg; }
};
struct Form {
    enum K { CONST, LIT, AND, OR, SET } k = CONST;
    int c = 0;
    Lit lit{-1, false};
    std::vector<Lit> lits;
    int pos = -1;           // SET: content position
    std::bitset<256> set;   // SET: the characters for which the form is 1
};

// what leads a hash-consing key: one class of gates each
enum KeyTag : int64_t {
    KEY_NIBBLE = 1,         // kind, pos, half, v, tag
    KEY_THRESHOLD = 2,      // is_and, literals
    KEY_CMP = 3,            // op, pos, c, tag
    KEY_EQ = 4,             // pos, c
    KEY_FAITHFUL_PAIR = 5,  // is_and, the DAG node: one gate per reference op
    KEY_SET_PRODUCT = 7,    // the two class gates, columns, LUT
    KEY_TREE_PAIR = 9,      // is_and, chain root, k-th join of the chain
};

struct KeyHash {  // FNV-1a over the words of a gate key
    size_t operator()(const std::vector<int64_t>& k) const {
        uint64_t h = 1469598103934665603ULL;
        for (int64_t w : k) h = (h ^ (uint64_t)w) * 1099511628211ULL;
        return (size_t)h;
    }
};
struct SetKey {
    int pos;
    std::bitset<256> set;
    bool operator==(const SetKey& o) const { return pos == o.pos && set == o.set; }
};
struct SetKeyHash {
    size_t operator()(const SetKey& k) const { return std::hash<std::bitset<256>>()(k.set) * 1000003u + (size_t)k.pos; }
};

struct Lowerer {
    const ValueDag& dag;
    int mode;
    Program prog;
    std::unordered_map<std::vector<int64_t>, int, KeyHash> gate_index;  // hash-consing of gates
    // expand_set results by (position, set): lowering a set creates its gates once
    // (later calls only hit gate_index), so the memo returns identical forms
    std::unordered_map<SetKey, Form, SetKeyHash> set_memo;
    std::vector<Form> memo;
    std::vector<char> done;

    Lowerer(const ValueDag& d, int m) : dag(d), mode(m), memo(d.nodes.size()), done(d.nodes.size(), 0) {
        const size_t hint = std::min<size_t>(2 * d.nodes.size(), (size_t)1 << 18);  // bounded for huge DAGs
        gate_index.reserve(hint);
        set_memo.reserve(hint / 2);
        prog.gates.reserve(hint);
    }

    int add_gate(std::vector<int64_t>&& key, PGate&& g) {
        auto it = gate_index.find(key);
        if (it != gate_index.end()) return it->second;
        prog.gates.push_back(std::move(g));
        int id = (int)prog.gates.size() - 1;
        gate_index.emplace(std::move(key), id);
        return id;
    }
    // [x_{2h} + 4 x_{2h+1} ? v] over the packed nibble of char `pos`
    int nibble_gate(int kind, int pos, int half, int v, int tag) {
        return add_gate({KEY_NIBBLE, kind, pos, half, v, tag}, nibble_test_gate(kind != 0, pos, half, v));
    }
    // arbitrary 16-entry LUT over the packed nibble (x_{2h} + 4 x_{2h+1}) of char `pos`
    // (its own index, keyed without a heap-allocated key: the lowering's most frequent lookup)
    struct NibKey {
        int32_t pos, half;
        uint64_t lut_lo, lut_hi;  // the 16 LUT bytes
        bool operator==(const NibKey& o) const {
            return pos == o.pos && half == o.half && lut_lo == o.lut_lo && lut_hi == o.lut_hi;
        }
    };
    struct NibKeyHash {
        size_t operator()(const NibKey& k) const {
            uint64_t h = (uint64_t)(uint32_t)k.pos * 0x9E3779B97F4A7C15ULL ^ (uint64_t)k.half;
            h = (h ^ k.lut_lo) * 0xBF58476D1CE4E5B9ULL;
            h = (h ^ k.lut_hi) * 0x94D049BB133111EBULL;
            return (size_t)(h ^ (h >> 31));
        }
    };
    std::unordered_map<NibKey, int, NibKeyHash> nib_index;
    int nibble_lut_gate(int pos, int half, const uint8_t* lut) {
        NibKey key{pos, half, 0, 0};
        std::memcpy(&key.lut_lo, lut, 8);
        std::memcpy(&key.lut_hi, lut + 8, 8);
        auto it = nib_index.find(key);
        if (it != nib_index.end()) return it->second;
        PGate g;
        g.ins = {{cblk(pos, 2 * half), 1}, {cblk(pos, 2 * half + 1), 4}};
        std::memcpy(g.lut, lut, 16);
        prog.gates.push_back(std::move(g));
        const int id = (int)prog.gates.size() - 1;
        nib_index.emplace(key, id);
        return id;
    }
    // Lower "char at pos is in S" (S != {} and S != all).  Characters split into
    // nibbles (hi, lo); rows = hi values grouped by their lo-set, columns = lo
    // values grouped by their hi-set.
    //  * product set (one non-empty row class): AND{[hi in H], [lo in L]} — two
    //    nibble PBS, mergeable into a parent AND;
    //  * rows x cols <= 16: two class LUTs + one PBS on (cols*row + col);
    //  * otherwise OR over row classes of AND{[hi in class], [lo in L_class]}.
    // index of signature `sig` among the classes, appended if new
    static int class_index(std::vector<std::bitset<16>>& cls, const std::bitset<16>& sig) {
        for (size_t i = 0; i < cls.size(); ++i)
            if (cls[i] == sig) return (int)i;
        cls.push_back(sig);
        return (int)cls.size() - 1;
    }
    Form lower_set(int pos, const std::bitset<256>& S) {
        // row h = bits 16h..16h+15 of S, read a 64-bit word at a time
        std::bitset<16> rowset[16];
        {
            const std::bitset<256> m64(~0ull);
            for (int w = 0; w < 4; ++w) {
                const unsigned long long word = ((S >> (64 * w)) & m64).to_ullong();
                for (int q = 0; q < 4; ++q) rowset[4 * w + q] = std::bitset<16>((word >> (16 * q)) & 0xFFFFu);
            }
        }
        // row classes: distinct non-empty lo-sets (class 0 = empty)
        std::vector<std::bitset<16>> rc;
        int rowcls[16];
        for (int h = 0; h < 16; ++h) rowcls[h] = rowset[h].none() ? 0 : class_index(rc, rowset[h]) + 1;
        if (rc.size() == 1) {  // product set
            uint8_t lh[16], ll[16];
            bool allh = true, alll = true;
            for (int v = 0; v < 16; ++v) {
                lh[v] = (uint8_t)(rowcls[v] != 0);
                ll[v] = (uint8_t)rc[0][v];
                allh &= lh[v] != 0;
                alll &= ll[v] != 0;
            }
            Form f;
            f.k = Form::AND;
            if (!allh) f.lits.push_back(Lit{nibble_lut_gate(pos, 1, lh), false});
            if (!alll) f.lits.push_back(Lit{nibble_lut_gate(pos, 0, ll), false});
            std::sort(f.lits.begin(), f.lits.end());
            if (f.lits.size() == 1) return lit_form(f.lits[0]);
            return f;
        }
        // column classes: distinct hi-sets of each lo value
        std::vector<std::bitset<16>> cc;
        int colcls[16];
        for (int l = 0; l < 16; ++l) {
            std::bitset<16> sig;
            for (int h = 0; h < 16; ++h) sig[h] = rowset[h][l];
            colcls[l] = class_index(cc, sig);
        }
        const int R = (int)rc.size() + 1, Cn = (int)cc.size();
        if (R * Cn <= 16) {
            uint8_t lh[16], ll[16];
            for (int v = 0; v < 16; ++v) {
                lh[v] = (uint8_t)rowcls[v];
                ll[v] = (uint8_t)colcls[v];
            }
            int gh = nibble_lut_gate(pos, 1, lh), gl = nibble_lut_gate(pos, 0, ll);
            PGate g;
            g.ins = {{gh, Cn}, {gl, 1}};
            for (int v = 0; v < 16; ++v) {
                int r = v / Cn, c = v % Cn;
                // representative hi for row class r, lo for column class c
                int member = 0;
                if (r >= 1 && r < R)
                    for (int l = 0; l < 16; ++l)
                        if (colcls[l] == c) { member = rc[r - 1][l]; break; }
                g.lut[v] = (uint8_t)member;
            }
            std::vector<int64_t> key{KEY_SET_PRODUCT, gh, gl, Cn};
            for (int v = 0; v < 16; ++v) key.push_back(g.lut[v]);
            return lit_form(Lit{add_gate(std::move(key), std::move(g)), false});
        }
        Form f;
        f.k = Form::OR;
        for (size_t r = 0; r < rc.size(); ++r) {
            uint8_t lh[16], ll[16];
            for (int v = 0; v < 16; ++v) {
                lh[v] = (uint8_t)(rowcls[v] == (int)r + 1);
                ll[v] = (uint8_t)rc[r][v];
            }
            std::vector<Lit> a{Lit{nibble_lut_gate(pos, 1, lh), false}, Lit{nibble_lut_gate(pos, 0, ll), false}};
            f.lits.push_back(Lit{threshold_gate(true, a), false});
        }
        std::sort(f.lits.begin(), f.lits.end());
        return f;
    }
    // SET -> general form (cheaper of S and its complement)
    Form expand_set(const Form& f) {
        if (f.set.none()) return const_form(0);
        if (f.set.all()) return const_form(1);
        const SetKey key{f.pos, f.set};
        auto it = set_memo.find(key);
        if (it != set_memo.end()) return it->second;
        Form r = expand_set_uncached(f);
        set_memo.emplace(key, r);
        return r;
    }
    Form expand_set_uncached(const Form& f) {
        Form a = lower_set(f.pos, f.set);
        if (a.k == Form::AND || a.k == Form::LIT) return a;
        Form b = negate(lower_set(f.pos, ~f.set));
        if (b.k == Form::AND || b.k == Form::LIT) return b;
        return a;
    }
    // AND / OR of m <= 16 literals as one SIGN gate:
    //   AND: s = sum - m + 1/2 > 0 ;  OR: s = sum - 1/2 > 0   (s in (-16, 16))
    int threshold_gate(bool is_and, std::vector<Lit> lits) {
        std::sort(lits.begin(), lits.end());
        PGate g;
        g.kind = GATE_SIGN;
        int negs = 0;
        std::vector<int64_t> key{KEY_THRESHOLD, is_and ? 1 : 0};
        for (auto& l : lits) {
            g.ins.push_back({l.gate, l.neg ? -1 : 1});
            negs += l.neg;
            key.push_back(l.gate * 2 + l.neg);
        }
        const int m = (int)lits.size();
        g.offset = 2 * negs + (is_and ? 1 - 2 * m : -1);
        return add_gate(std::move(key), std::move(g));
    }
    Lit materialize(const Form& f0) {
        if (f0.k == Form::SET) return materialize(expand_set(f0));
        const Form& f = f0;
        if (f.k == Form::LIT) return f.lit;
        if (f.k == Form::CONST) throw Error(FR_ERR_INVALID, "lowering: cannot materialize a constant");
        bool is_and = f.k == Form::AND;
        std::vector<Lit> lits = reduce(is_and, f.lits, MAX_FANIN);
        if (lits.size() == 1) return lits[0];
        return Lit{threshold_gate(is_and, lits), false};
    }
    // levels of threshold gates (fan-in <= 16, balanced chunks) until <= keep literals remain
    std::vector<Lit> reduce(bool is_and, std::vector<Lit> lits, size_t keep) {
        while (lits.size() > keep) {
            std::vector<Lit> next;
            for_balanced_chunks(lits.size(), [&](size_t start, size_t len) {
                std::vector<Lit> part(lits.begin() + start, lits.begin() + start + len);
                next.push_back(len == 1 ? part[0] : Lit{threshold_gate(is_and, part), false});
            });
            lits = std::move(next);
        }
        return lits;
    }
    // the parts of a root: an OR form's literals reduced to <= max_parts, else one literal
    std::vector<Lit> parts(const Form& f0, size_t max_parts) {
        if (f0.k == Form::SET) return parts(expand_set(f0), max_parts);
        if (f0.k == Form::OR && max_parts > 1) return reduce(false, f0.lits, max_parts);
        return {materialize(f0)};
    }
    static Form lit_form(Lit l) {
        Form f;
        f.k = Form::LIT;
        f.lit = l;
        return f;
    }
    static Form const_form(int c) {
        Form f;
        f.k = Form::CONST;
        f.c = c;
        return f;
    }
    // literals of f as members of an AND (is_and) or OR list
    // (f is consumed: a same-kind form hands over its literal list)
    std::vector<Lit> members(Form&& f, bool is_and) {
        if (f.k == Form::SET) return members(expand_set(f), is_and);
        if (f.k == Form::CONST) throw Error(FR_ERR_INVALID, "lowering: constant member");
        if (f.k == Form::LIT) return {f.lit};
        if ((f.k == Form::AND) == is_and) return std::move(f.lits);
        return {materialize(f)};
    }
    // operands by value: lower_t moves a node's form in at its last use, so the long
    // AND/OR chains of has_match grow their literal lists without copies
    Form combine(bool is_and, Form a0, Form b0) {
        // same-position character sets combine exactly
        if (a0.k == Form::SET && b0.k == Form::SET && a0.pos == b0.pos) {
            Form f = std::move(a0);
            f.set = is_and ? (f.set & b0.set) : (f.set | b0.set);
            if (f.set.none()) return const_form(0);
            if (f.set.all()) return const_form(1);
            return f;
        }
        Form a = a0.k == Form::SET ? expand_set(a0) : std::move(a0);
        Form b = b0.k == Form::SET ? expand_set(b0) : std::move(b0);
        // constant folding (booleans)
        if (a.k == Form::CONST) return is_and ? (a.c ? std::move(b) : const_form(0)) : (a.c ? const_form(1) : std::move(b));
        if (b.k == Form::CONST) return is_and ? (b.c ? std::move(a) : const_form(0)) : (b.c ? const_form(1) : std::move(a));
        // member lists are sorted (forms keep their literals sorted): merge, O(|a|+|b|)
        std::vector<Lit> l0 = members(std::move(a), is_and), r = members(std::move(b), is_and);
        if (l0.size() < r.size()) std::swap(l0, r);
        if (r.size() == 1) {
            // the long folds (has_match's OR over its branches, engine.rs:22-35) add one
            // literal at a time, usually past the end: insert in place instead of copying
            // the whole list per operand (quadratic in the branch count)
            // (a form's own list is sorted, unique and free of x / !x pairs: only x's
            // neighbours can complement it)
            const Lit x = r[0];
            auto it = std::lower_bound(l0.begin(), l0.end(), x);
            if (it == l0.end() || !(*it == x)) {
                if ((it != l0.end() && it->gate == x.gate) || (it != l0.begin() && (it - 1)->gate == x.gate))
                    return const_form(is_and ? 0 : 1);  // x & !x, x | !x
                l0.insert(it, x);
            }
            if (l0.size() == 1) return lit_form(l0[0]);
            Form f;
            f.k = is_and ? Form::AND : Form::OR;
            f.lits = std::move(l0);
            return f;
        }
        std::vector<Lit> l;
        l.reserve(l0.size() + r.size());
        std::merge(l0.begin(), l0.end(), r.begin(), r.end(), std::back_inserter(l));
        l.erase(std::unique(l.begin(), l.end()), l.end());
        for (size_t i = 0; i + 1 < l.size(); ++i)
            if (l[i].gate == l[i + 1].gate) return const_form(is_and ? 0 : 1);  // x & !x, x | !x
        if (l.size() == 1) return lit_form(l[0]);
        Form f;
        f.k = is_and ? Form::AND : Form::OR;
        f.lits = std::move(l);
        return f;
    }
    Form negate(const Form& f) {
        Form g = f;
        switch (f.k) {
            case Form::SET: g.set = ~f.set; break;
            case Form::CONST: g.c = f.c ^ 1; break;
            case Form::LIT: g.lit.neg = !f.lit.neg; break;
            case Form::AND:
            case Form::OR:
                g.k = f.k == Form::AND ? Form::OR : Form::AND;
                for (auto& l : g.lits) l.neg = !l.neg;
                break;
        }
        return g;
    }

    // ---------------------------------------------------------- the walk
    // Post-order over the AND/OR/NOT operands below `id` (iterative: the chains of
    // has_match are deep), memoised.  A content char and a constant are the same in every
    // lowering; every other node's form is visit(x, node), called once its operands are done.
    template <class Visit>
    const Form& walk(int id, Visit&& visit) {
        std::vector<int> st{id};
        while (!st.empty()) {
            int x = st.back();
            if (done[x]) { st.pop_back(); continue; }
            const VNode& n = dag.nodes[x];
            bool ready = true;
            if ((n.op == VNode::AND || n.op == VNode::OR || n.op == VNode::NOT)) {
                if (!done[n.a]) { st.push_back(n.a); ready = false; }
                if (n.b >= 0 && !done[n.b]) { st.push_back(n.b); ready = false; }
            }
            if (!ready) continue;
            st.pop_back();
            if (n.op == VNode::POS) throw Error(FR_ERR_INVALID, "lowering: content char used as a boolean");
            Form f = n.op == VNode::CONST ? const_form(n.c) : visit(x, n);
            memo[x] = std::move(f);
            done[x] = 1;
        }
        return memo[id];
    }

    // ---------------------------------------------------------- threshold
    std::vector<int32_t> uses;  // remaining AND/OR/NOT operand uses of each node (lower_t)
    Form take(int id) {
        if (--uses[id] <= 0) return std::move(memo[id]);
        return memo[id];
    }
    Form lower_t(int id) {
        if (done[id]) return memo[id];
        uses.assign(dag.nodes.size(), 0);
        for (const VNode& n : dag.nodes)
            if (n.op == VNode::AND || n.op == VNode::OR) {
                ++uses[n.a];
                ++uses[n.b];
            } else if (n.op == VNode::NOT) {
                ++uses[n.a];
            }
        ++uses[id];  // the root's form is returned
        return walk(id, [&](int, const VNode& n) {
            if (n.op == VNode::NOT) return negate(take(n.a));
            if (n.op == VNode::AND || n.op == VNode::OR) {
                Form fa = take(n.a);
                return combine(n.op == VNode::AND, std::move(fa), take(n.b));
            }
            Form f;  // EQ / GT / LE
            f.k = Form::SET;
            f.pos = n.pos;
            // {c}, {ch > c} or {ch <= c}, built word-wise
            const std::bitset<256> all = std::bitset<256>().set();
            if (n.op == VNode::EQ) f.set.reset().set(n.c);
            else if (n.op == VNode::GT) f.set = all << (n.c + 1);
            else f.set = all >> (255 - n.c);
            return f;
        });
    }

    // ---------------------------------------------------------- faithful
    // eq (smart_eq): both nibble tests, low first, then [lo + hi == 2]; gt / le: both sign
    // tests, high first, then lut_gt3  (3 PBS each)
    Form cmp_form(const VNode& n) {
        const int tag = n.c;
        int lo, hi;
        if (n.op == VNode::EQ) {
            lo = nibble_gate(0, n.pos, 0, n.c & 15, tag);
            hi = nibble_gate(0, n.pos, 1, n.c >> 4, tag);
        } else {
            hi = nibble_gate(1, n.pos, 1, n.c >> 4, tag);
            lo = nibble_gate(1, n.pos, 0, n.c & 15, tag);
        }
        std::vector<int64_t> key = n.op == VNode::EQ ? std::vector<int64_t>{KEY_EQ, n.pos, n.c}
                                                     : std::vector<int64_t>{KEY_CMP, n.op, n.pos, n.c, tag};
        return lit_form(Lit{add_gate(std::move(key), cmp_final_gate(n.op, lo, hi)), false});
    }
    // a faithful operand: its constant, or its literal
    PairOperand operand(const Form& o) {
        if (o.k == Form::CONST) return PairOperand{-1, false, o.c};
        const Lit l = materialize(o);
        return PairOperand{l.gate, l.neg, 0};
    }
    // one gate group per distinct reference op
    Form lower_f(int id) {
        return walk(id, [&](int x, const VNode& n) {
            if (n.op == VNode::NOT) return negate(memo[n.a]);  // smart_bitxor(a, 1) on a boolean: linear
            if (n.op != VNode::AND && n.op != VNode::OR) return cmp_form(n);
            const bool is_and = n.op == VNode::AND;
            const PairOperand a = operand(memo[n.a]), b = operand(memo[n.b]);
            return lit_form(Lit{add_gate({KEY_FAITHFUL_PAIR, is_and, x}, pair_gate(is_and, a, b)), false});
        });
    }

    // ---------------------------------------------------------- faithful tree
    // The faithful gates with the reference's AND/OR chains rebalanced.
    // A chain is a maximal run of AND (or OR) nodes in which every inner node is used
    // once, by the next node of the same op: the left fold of has_match
    // (engine.rs:22-35) and the Seq / Repeated AND chains (engine.rs:127-211).  A chain
    // over m operands keeps exactly m - 1 two-input gates, as lower_f makes one per node
    // (the reference's PBS count), but they form a tree of least depth: the two
    // shallowest operands are joined first (ties in operand order).  A constant operand
    // (or(false, x) is not short-circuited, execution.rs:154-164) is joined to the
    // shallowest other operand as the same trivial-offset gate lower_f makes.
    std::vector<int32_t> glv;  // level of each gate so far
    int level_of(int g) {
        for (int i = (int)glv.size(); i <= g; ++i) glv.push_back(gate_level(prog.gates[i], [&](int s) { return glv[s]; }));
        return glv[g];
    }
    Form lower_ft(int id) {
        const size_t nn = dag.nodes.size();
        std::vector<int32_t> nuse(nn, 0), user(nn, -1);
        for (size_t x = 0; x < nn; ++x) {
            const VNode& n = dag.nodes[x];
            if (n.op == VNode::AND || n.op == VNode::OR) {
                ++nuse[n.a], user[n.a] = (int)x;
                ++nuse[n.b], user[n.b] = (int)x;
            } else if (n.op == VNode::NOT) {
                ++nuse[n.a], user[n.a] = (int)x;
            }
        }
        ++nuse[id];  // the root is used by the result
        auto absorbed = [&](int x) {
            const VNode& n = dag.nodes[x];
            return (n.op == VNode::AND || n.op == VNode::OR) && nuse[x] == 1 && user[x] >= 0 &&
                   dag.nodes[user[x]].op == n.op;
        };
        return walk(id, [&](int x, const VNode& n) {
            if (n.op == VNode::NOT) return negate(memo[n.a]);
            if (n.op != VNode::AND && n.op != VNode::OR) return cmp_form(n);  // lower_f's comparison gates
            if (absorbed(x)) return Form{};  // an inner link: its chain root gathers its operands
            const bool is_and = n.op == VNode::AND;
            // the chain's operands, left to right
            std::vector<PairOperand> leaves;
            std::vector<int> ds{n.b, n.a};
            while (!ds.empty()) {
                int y = ds.back();
                ds.pop_back();
                if (absorbed(y) && user[y] >= 0) {
                    ds.push_back(dag.nodes[y].b);
                    ds.push_back(dag.nodes[y].a);
                    continue;
                }
                leaves.push_back(operand(memo[y]));
            }
            // least-depth binary tree: join the two shallowest operands first
            using QE = std::tuple<int, int, int>;  // (level, order, item index)
            std::priority_queue<QE, std::vector<QE>, std::greater<QE>> q;
            std::vector<PairOperand> items;
            std::vector<PairOperand> consts;
            int order = 0;
            for (const PairOperand& it : leaves) {
                if (it.gate < 0) { consts.push_back(it); continue; }
                items.push_back(it);
                q.emplace(level_of(it.gate), order++, (int)items.size() - 1);
            }
            int k = 0;
            auto join = [&](const PairOperand& p, const PairOperand& r) {
                int g = add_gate({KEY_TREE_PAIR, is_and, x, k++}, pair_gate(is_and, p, r));
                items.push_back(PairOperand{g, false, 0});
                q.emplace(level_of(g), order++, (int)items.size() - 1);
            };
            size_t c0 = 0;
            if (q.empty()) {
                // every operand's value is a constant (a short-circuit returns its
                // operand under a new key, execution.rs:121-164, so the op above it is
                // real): lower_f's input-free gate, as the first join
                if (consts.size() < 2) throw Error(FR_ERR_INVALID, "lowering: one-operand chain");
                join(consts[0], consts[1]);
                c0 = 2;
            }
            for (size_t ci = c0; ci < consts.size(); ++ci) {
                const PairOperand c = consts[ci];
                const int ix = std::get<2>(q.top());
                q.pop();
                join(PairOperand(items[ix]), c);
            }
            while (q.size() > 1) {
                auto [l1, o1, i1] = q.top();
                q.pop();
                auto [l2, o2, i2] = q.top();
                q.pop();
                (void)l1, (void)l2;
                // operand order as in the chain (the earlier one first)
                const PairOperand p1 = items[i1], p2 = items[i2];
                if (o1 < o2) join(p1, p2);
                else join(p2, p1);
            }
            const PairOperand& top = items[std::get<2>(q.top())];
            return lit_form(Lit{top.gate, top.neg});
        });
    }
};

// drop the gates not reachable from the outputs (e.g. materialized then merged), renumbering the rest
Program sweep_dead_gates(Program&& p) {
    std::vector<char> live(p.gates.size(), 0);
    for (const ProgOut& o : p.outs) {
        if (o.gate < 0) continue;
        std::vector<int> st{o.gate};
        while (!st.empty()) {
            int g = st.back();
            st.pop_back();
            if (live[g]) continue;
            live[g] = 1;
            for (auto& in : p.gates[g].ins)
                if (in.src >= 0 && !live[in.src]) st.push_back(in.src);
        }
    }
    std::vector<int> remap(p.gates.size(), -1);
    Program out;
    for (size_t g = 0; g < p.gates.size(); ++g) {
        if (!live[g]) continue;
        PGate ng = std::move(p.gates[g]);
        for (auto& in : ng.ins)
            if (in.src >= 0) in.src = remap[in.src];
        remap[g] = (int)out.gates.size();
        out.gates.push_back(std::move(ng));
    }
    for (ProgOut o : p.outs) {
        if (o.gate >= 0) o.gate = remap[o.gate];
        out.outs.push_back(o);
    }
    return out;
}

}  // namespace

void compute_levels(Program& prog) {
    int maxl = 0;
    std::vector<size_t> width;
    for (auto& g : prog.gates) {
        g.level = gate_level(g, [&](int s) { return prog.gates[s].level; });
        if (g.level == 0) continue;  // an extract-sum: no bootstrap, in no level's width
        maxl = std::max(maxl, g.level);
        if ((size_t)g.level >= width.size()) width.resize(g.level + 1, 0);
        width[g.level]++;
    }
    prog.levels = maxl;
    prog.max_width = 0;
    for (auto w : width) prog.max_width = std::max(prog.max_width, w);
}

Program lower(const ValueDag& dag, int root, int mode, int max_parts) {
    if (max_parts < 1 || max_parts > MAX_FANIN) throw Error(FR_ERR_INVALID, "lowering: parts must be in [1, 16]");
    Lowerer lw(dag, mode);
    Form f = mode == FR_LOWER_FAITHFUL ? lw.lower_f(root)
             : mode == FR_LOWER_FAITHFUL_TREE ? lw.lower_ft(root) : lw.lower_t(root);
    Program& p = lw.prog;
    if (f.k == Form::SET) f = lw.expand_set(f);  // (an empty or full set is a constant)
    if (f.k == Form::CONST) {
        p.outs.push_back(ProgOut{-1, 0, f.c});
    } else {
        for (const Lit& l : lw.parts(f, (size_t)max_parts))
            p.outs.push_back(ProgOut{l.gate, l.neg ? -1 : 1, l.neg ? 1 : 0});
    }
    Program out = sweep_dead_gates(std::move(p));
    compute_levels(out);
    return out;
}

CompiledMatch compile_match(const MatchSpec& s) {
    CompiledMatch m;
    const ReP re = parse(s.pattern, s.grammar);  // engine.rs:13
    m.rec = record_has_match_engine(m.dag, s.n_chars, re, s.lo, s.hi, s.engine);
    m.prog = lower(m.dag, m.rec.root, s.lowering, s.parts);
    return m;
}

CompiledStarts compile_match_starts(const MatchSpec& s, bool keep_dags) {
    CompiledStarts m;
    const ReP re = parse(s.pattern, s.grammar);  // engine.rs:13 (an empty range lo >= hi: no start)
    // structure of a merged gate (its inputs already remapped) -> its index
    std::map<std::string, int32_t> seen;
    auto structure = [](const PGate& g) {
        std::string k((const char*)g.lut, 16);
        auto put = [&](int32_t v) { k.append((const char*)&v, 4); };
        put(g.offset);
        put(g.kind);
        for (const PIn& in : g.ins) put(in.src), put(in.w);
        return k;
    };
    Program& out = m.prog;
    for (size_t st = s.lo; st < s.hi; ++st) {
        ValueDag dag;
        const Recorded rec = record_has_match_engine(dag, s.n_chars, re, st, st + 1, s.engine);
        const Program p = lower(dag, rec.root, s.lowering, 1);
        m.rec.ct_ops += rec.ct_ops;
        m.rec.cache_hits += rec.cache_hits;
        m.rec.n_branches += rec.n_branches;
        std::vector<int32_t> at(p.gates.size());  // gate of p -> merged gate
        for (size_t g = 0; g < p.gates.size(); ++g) {
            PGate G = p.gates[g];
            for (PIn& in : G.ins)
                if (in.src >= 0) in.src = at[(size_t)in.src];
            const auto ins = seen.emplace(structure(G), (int32_t)out.gates.size());
            if (ins.second) out.gates.push_back(std::move(G));
            at[g] = ins.first->second;
        }
        ProgOut o = p.outs.at(0);
        if (o.gate >= 0) o.gate = at[(size_t)o.gate];
        out.outs.push_back(o);
        if (keep_dags) {
            m.roots.push_back(rec.root);
            m.dags.push_back(std::move(dag));
        }
    }
    compute_levels(out);
    return m;
}

// AND / OR of the gates `lits` as a balanced tree of threshold gates (threshold_gate's offsets,
// no negations), appended to prog; the root's index (one literal: itself)
static int threshold_tree(Program& prog, bool is_and, std::vector<int> lits) {
    while (lits.size() > 1) {
        std::vector<int> next;
        for_balanced_chunks(lits.size(), [&](size_t start, size_t len) {
            if (len == 1) {
                next.push_back(lits[start]);
                return;
            }
            PGate g;
            g.kind = GATE_SIGN;
            for (size_t i = 0; i < len; ++i) g.ins.push_back({lits[start + i], 1});
            g.offset = is_and ? 1 - 2 * (int)len : -1;
            next.push_back((int)prog.gates.size());
            prog.gates.push_back(std::move(g));
        });
        lits = std::move(next);
    }
    return lits[0];
}

// stride: the content position of start p's first character is p * stride (1: the text itself;
// m, clear only: window p of a compacted text, compile_needle_windows)
static Program compile_needle_over(size_t n_chars, size_t m, size_t lo, size_t hi, bool starts, bool clear,
                                   size_t stride = 1, bool bytes = false) {
    if (m < 1 || m > NEEDLE_MAX_CHARS) throw Error(FR_ERR_INVALID, "needle: 1 <= m <= 64");
    if (lo > hi) throw Error(FR_ERR_INVALID, "needle: start range");
    if (n_chars > (size_t)1 << 24) throw Error(FR_ERR_INVALID, "needle: content too long");
    if (starts && hi - lo > (size_t)1 << 24) throw Error(FR_ERR_INVALID, "needle: more than 2^24 starts");
    // (the OR reads only starts that fit: no walk over a range far past the content)
    const size_t end = starts ? hi : std::min(hi, n_chars);
    Program prog;
    std::vector<int> found;  // the AND of each start that fits
    for (size_t p = lo; p < end; ++p) {
        const size_t at = p * stride;  // (p < 2^24 and stride <= 64: no overflow)
        if (at + m > n_chars || at + m < at) {
            if (starts) prog.outs.push_back(ProgOut{-1, 0, 0});
            continue;
        }
        std::vector<int> tests;
        if (clear) {
            // test 2 i + h is a term; a chunk of them, summed, feeds the SIGN gate that would AND them
            // (a byte-table needle: test i is the term of table i, m of them)
            for_balanced_chunks(bytes ? m : 2 * m, [&](size_t first, size_t len) {
                PGate sum;
                sum.kind = GATE_EXTRACT;
                for (size_t t = first; t < first + len; ++t)
                    if (bytes) sum.terms.push_back({(int32_t)t, (int32_t)(at + t), 0});
                    else sum.terms.push_back({(int32_t)t, (int32_t)(at + t / 2), (int32_t)(t % 2)});
                PGate g;
                g.kind = GATE_SIGN;
                g.ins = {{(int32_t)prog.gates.size(), 1}};
                g.offset = 1 - 2 * (int)len;
                prog.gates.push_back(std::move(sum));
                tests.push_back((int)prog.gates.size());
                prog.gates.push_back(std::move(g));
            });
        } else {
            for (size_t i = 0; i < m; ++i)
                for (int h = 0; h < 2; ++h) {
                    PGate g;
                    g.kind = GATE_SELECT;
                    g.sel = (int32_t)(2 * i + h);
                    g.ins = {{cblk((int)(p + i), 2 * h + 1), 4}, {cblk((int)(p + i), 2 * h), 1}};
                    tests.push_back((int)prog.gates.size());
                    prog.gates.push_back(std::move(g));
                }
        }
        const int a = threshold_tree(prog, true, std::move(tests));
        if (starts) prog.outs.push_back(ProgOut{a, 1, 0});
        else found.push_back(a);
    }
    if (!starts) {
        if (found.empty()) prog.outs.push_back(ProgOut{-1, 0, 0});
        else prog.outs.push_back(ProgOut{threshold_tree(prog, false, std::move(found)), 1, 0});
    }
    // topological order by construction, but a tree's gates follow their start's tests: the
    // scheduler orders by level, and level 1 is the selector gates alone (clear: the sign gates
    // over the sums, which are level 0)
    compute_levels(prog);
    return prog;
}

Program compile_needle(size_t n_chars, size_t m, size_t lo, size_t hi, bool starts) {
    return compile_needle_over(n_chars, m, lo, hi, starts, false);
}
Program compile_needle_clear(size_t n_chars, size_t m, size_t lo, size_t hi, bool starts, bool bytes) {
    return compile_needle_over(n_chars, m, lo, hi, starts, true, 1, bytes);
}
Program compile_needle_windows(size_t n_windows, size_t m, bool starts, bool bytes) {
    if (m < 1 || m > NEEDLE_MAX_CHARS) throw Error(FR_ERR_INVALID, "needle: 1 <= m <= 64");
    if (n_windows > ((size_t)1 << 24) / m) throw Error(FR_ERR_INVALID, "scan: more than 2^24 window bytes");
    return compile_needle_over(n_windows * m, m, 0, n_windows, starts, true, m, bytes);
}
Program needle_program(MatchKind kind, size_t n, size_t m, size_t lo, size_t hi, bool starts, bool bytes) {
    switch (kind) {
        case MATCH_NEEDLE:
            if (bytes) throw Error(FR_ERR_INVALID, "needle: a byte-table needle searches clear content only");
            return compile_needle(n, m, lo, hi, starts);
        case MATCH_NEEDLE_CLEAR: return compile_needle_clear(n, m, lo, hi, starts, bytes);
        case MATCH_NEEDLE_WINDOWS: return compile_needle_windows(n, m, starts, bytes);
        default: throw Error(FR_ERR_INVALID, "a pattern match has no needle program");
    }
}

void pad_window_text(WindowClasses& wc, size_t m) {
    if (wc.first.empty()) return;
    const std::vector<uint8_t> w0(wc.text.begin(), wc.text.begin() + (long)m);
    for (size_t d = wc.first.size(); d < scan_padded(wc.first.size()); ++d)
        wc.text.insert(wc.text.end(), w0.begin(), w0.end());
}

WindowClasses window_classes(const uint8_t* text, size_t n, size_t m, size_t lo, size_t hi) {
    if (m < 1 || m > NEEDLE_MAX_CHARS) throw Error(FR_ERR_INVALID, "needle: 1 <= m <= 64");
    if (lo > hi) throw Error(FR_ERR_INVALID, "needle: start range");
    WindowClasses wc;
    const size_t end = std::min(hi, n);
    wc.cls.assign(end > lo ? end - lo : 0, -1);
    // the window's bytes are the key: equal hashes alone never make two windows one class
    std::unordered_map<std::string_view, int32_t> seen;
    const char* t = (const char*)text;
    for (size_t p = lo; p < end && p + m <= n; ++p) {
        const auto ins = seen.emplace(std::string_view(t + p, m), (int32_t)seen.size());
        if (ins.second) wc.first.push_back(p);
        wc.cls[p - lo] = ins.first->second;
    }
    wc.text.reserve(wc.first.size() * m);
    for (size_t p : wc.first) wc.text.insert(wc.text.end(), text + p, text + p + m);
    return wc;
}

int eval_program(const Program& prog, const uint8_t* content, size_t L) {
    std::vector<int> parts;
    return eval_program_parts(prog, content, L, parts);
}

int eval_program_parts(const Program& prog, const uint8_t* content, size_t L, std::vector<int>& parts,
                       const uint16_t* tables, size_t n_tables, const uint8_t* byte_tables) {
    std::vector<int> val(prog.gates.size(), 0);
    for (size_t g = 0; g < prog.gates.size(); ++g) {
        const PGate& G = prog.gates[g];
        if (G.kind == GATE_EXTRACT) {
            for (const PTerm& t : G.terms) {
                if (t.sel < 0 || (size_t)t.sel >= n_tables) throw Error(FR_ERR_INVALID, "extract-sum without its table");
                if (t.pos < 0 || (size_t)t.pos >= L) throw Error(FR_ERR_INVALID, "program references content past its end");
                if (byte_tables) val[g] += (byte_tables[32 * (size_t)t.sel + content[t.pos] / 8] >> (content[t.pos] % 8)) & 1;
                else val[g] += (tables[t.sel] >> ((content[t.pos] >> (4 * (t.half & 1))) & 15)) & 1;
            }
            continue;
        }
        int s = G.offset;  // half units
        for (auto& in : G.ins) {
            int v;
            if (in.src >= 0) {
                v = val[in.src];
            } else {
                int cb = -in.src - 1;
                size_t pos = (size_t)(cb / 4);
                if (pos >= L) throw Error(FR_ERR_INVALID, "program references content past its end");
                v = (content[pos] >> (2 * (cb % 4))) & 3;
            }
            s += 2 * in.w * v;
        }
        if (G.kind == GATE_SIGN) {
            if ((s & 1) == 0 || s <= -32 || s >= 32) throw Error(FR_ERR_INVALID, "sign gate input out of (-16, 16) or integral");
            val[g] = s > 0 ? 1 : 0;
        } else {
            if ((s & 1) || s < 0 || s >= 32) throw Error(FR_ERR_INVALID, "program lincomb out of the 16-value message space");
            if (G.kind == GATE_SELECT) {
                if (G.sel < 0 || (size_t)G.sel >= n_tables) throw Error(FR_ERR_INVALID, "selector gate without its table");
                val[g] = (tables[G.sel] >> (s / 2)) & 1;
                continue;
            }
            val[g] = G.lut[s / 2];
        }
    }
    parts.clear();
    int any = 0;
    for (const ProgOut& o : prog.outs) {
        parts.push_back(o.gate < 0 ? o.cst : o.cst + o.w * val[o.gate]);
        any |= parts.back();
    }
    return any;
}

}  // namespace fr
