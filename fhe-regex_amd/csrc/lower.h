// Lowering of the recorded value DAG (what the reference computes through
// tfhe-rs smart_* calls) into a program of programmable bootstraps (PBS).
//
// Every gate is one programmable bootstrap of  s = offset/2 + sum_i w_i * in_i
// (offset in units of Delta/2, Delta = 2^59).  Inputs are content blocks (2-bit
// radix digits of the encrypted characters, src/regex/ciphertext.rs:18-29) or
// earlier gates.  Two kinds:
//  * LUT  : s integral in [0, 16), out = lut[s] (16-box test polynomial, one
//           padding bit, as tfhe-rs shortint PARAM_MESSAGE_2_CARRY_2);
//  * SIGN : s half-integral in (-16, 16), out = [s > 0] (constant test
//           polynomial: the negacyclic rotation yields +-Delta/2, then +Delta/2).
//           Threshold AND/OR of up to 16 literals in one bootstrap.
//  * SELECT : a LUT gate whose table the server does not know (private search): out =
//           T_sel[s] for the 0/1 table T_sel that selector `sel` of the call's needle encrypts.
//           Inputs, offsets and level rule are a LUT gate's; the lut field is unused.
//  * EXTRACT : an extract-sum (private search over clear content): no bootstrap.  out = the
//           number of its terms (selector, content position, half) whose selector's table
//           accepts that nibble of the clear content, an integer in [0, 16], formed as a sum of
//           sample extracts of the selectors (device.h: DevSum).  No inputs, level 0: neither a
//           job nor a rotation; only SIGN gates read it (weight 1), as they would read its terms.
//           Over a byte-table needle (the form is the needle's, and so the bound selector table's,
//           never the gate's) a term is (table, content position, 0) and counts when the table
//           accepts that byte.
//
// FR_LOWER_FAITHFUL: one gate group per reference op (eq/gt/le = 3 PBS, and/or
//   = 1 PBS, not = linear), the decomposition of SURVEY App. D.3.
// FR_LOWER_THRESHOLD (default): AND/OR trees of the recorded circuit are
//   flattened into n-ary threshold gates (AND of m literals = [sum == m],
//   OR = [sum >= 1], m <= 15), NOT is pushed into literals (De Morgan, linear),
//   equality nibble tests are shared across constants.  Same decrypted result,
//   far fewer PBS and levels.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "regex.h"

namespace fr {

struct PIn {
    int32_t src;  // >= 0: gate index; < 0: content block -(1 + pos*4 + blk)
    int32_t w;
};
enum GateKind : int32_t { GATE_LUT = 0, GATE_SIGN = 1, GATE_SELECT = 2, GATE_EXTRACT = 3 };
// one term of an extract-sum: selector `sel` of the needle looks up nibble `half` (0: low) of the
// clear content byte at `pos`
struct PTerm {
    int32_t sel, pos, half;
};
struct PGate {
    std::vector<PIn> ins;
    int32_t offset = 0;  // units of Delta/2
    int32_t kind = GATE_LUT;
    uint8_t lut[16] = {0};
    int32_t level = 0;
    int32_t sel = 0;  // GATE_SELECT: the selector's index in the needle
    std::vector<PTerm> terms;  // GATE_EXTRACT: 1..16 of them
};
// one boolean output: cst + w * gates[gate]   (gate == -1: the constant cst)
struct ProgOut {
    int32_t gate = -1, w = 0, cst = 0;
};
struct Program {
    std::vector<PGate> gates;
    // the outputs: one boolean, or (lower's max_parts > 1) up to max_parts booleans whose
    // OR is the result
    std::vector<ProgOut> outs;
    int32_t levels = 0;
    size_t max_width = 0;
};

constexpr int MAX_FANIN = 16;

// max_parts > 1: a root OR (the has_match fold over start offsets, engine.rs:22-35)
// stops its threshold tree at <= max_parts literals and outputs them as parts, so the
// caller's own OR of several parts lists (start shards on several GPUs) is the
// tree's last level instead of one more.  Faithful lowerings and non-OR roots: one part.
Program lower(const ValueDag& dag, int root, int mode, int max_parts = 1);
// Plaintext semantics of a program (LUT semantics, with the [0,16) range
// check); returns the result value (several parts: their OR).
int eval_program(const Program& prog, const uint8_t* content, size_t L);
// the same, and each output's value in `parts`; tables (n_tables 16-bit masks of accepted
// values) are what the program's selector gates look up: bit s of tables[sel]; an extract-sum
// counts its terms with bit (content[pos] >> 4 half) & 15 of tables[sel] set.  byte_tables (a
// byte-table needle's program: n_tables sets of 256 bits, 32 bytes each, tables unused): an
// extract-sum counts its terms with bit content[pos] of byte table `sel` set.
int eval_program_parts(const Program& prog, const uint8_t* content, size_t L, std::vector<int>& parts,
                       const uint16_t* tables = nullptr, size_t n_tables = 0, const uint8_t* byte_tables = nullptr);
void compute_levels(Program& prog);
// a gate's level: one past its deepest gate input (content blocks are level 0, and so is an
// extract-sum, which is no bootstrap); level_of(g) gives the level of an earlier gate
template <class LevelOf>
int gate_level(const PGate& g, LevelOf&& level_of) {
    if (g.kind == GATE_EXTRACT) return 0;
    int l = 0;
    for (const PIn& in : g.ins)
        if (in.src >= 0) l = std::max(l, (int)level_of(in.src));
    return l + 1;
}

// The front end of every match: parse once, record under the engine, lower.  The error
// order is the stages': a parse error first, then the recording's (FR_ERR_OOM from the
// enumeration, the merged engine's refusals), then the lowering's.
struct MatchSpec {
    std::string pattern;
    size_t n_chars = 0, lo = 0, hi = 0;  // start offsets [lo, hi)
    int engine = FR_ENGINE_AUTO, grammar = FR_GRAMMAR_REFERENCE, lowering = FR_LOWER_THRESHOLD;
    int parts = 1;  // lower's max_parts
};
struct CompiledMatch {
    Recorded rec;
    Program prog;
    ValueDag dag;  // the recorded circuit (rec.root), for a plaintext evaluation
};
CompiledMatch compile_match(const MatchSpec& spec);

// Match starts: one boolean per start offset s of [lo, hi), the value the reference ORs away at
// engine.rs:22-35 (compile_match of [s, s + 1) with one part).  The per-start programs are
// merged into one with structural dedupe -- a gate with the (ins, offset, kind, lut) of an
// earlier one is that gate -- so the nibble tests of a content position are shared by every
// start that reads it, and everything above them transitively.  prog.outs[s - lo] is start s's
// output (gate == -1: a constant, e.g. /^abc/ at s > 0); rec sums the recordings' counters;
// keep_dags: dags[s - lo] / roots[s - lo] are start s's recorded circuit (a plaintext
// evaluation's; the execution path does not hold them).  Errors in compile_match's order, of
// the first start that has one.  spec.parts is not used; lo >= hi is no start at all.
struct CompiledStarts {
    Recorded rec;
    Program prog;
    std::vector<ValueDag> dags;
    std::vector<int> roots;
};
CompiledStarts compile_match_starts(const MatchSpec& spec, bool keep_dags = false);

// Private search: has-match (starts = false: one output, the OR over the starts) or match starts
// (one output per start of [lo, hi)) of a needle of m characters whose 2 m nibble tables are
// encrypted.  For every start p of the range with p + m <= n_chars: selector gates 2 i + h over
// nibble h (0: low) of content character p + i, then their AND.  A start that cannot fit is the
// constant 0, and so is the OR over no start.  1 <= m <= NEEDLE_MAX_CHARS (common.h); m > n_chars is no error.
// The program depends on (n_chars, m, lo, hi, starts) alone.  starts: at most 2^24 of them.
Program compile_needle(size_t n_chars, size_t m, size_t lo, size_t hi, bool starts);
// The same search over content the server holds in the clear: compile_needle with its selector
// layer replaced by extract-sums.  The AND of a start's 2 m tests is one SIGN gate over one
// extract-sum of 2 m terms (offset 1 - 2 len, as the AND over the tests themselves); for
// 2 m > 16 each balanced chunk of the tests gets its own sum and SIGN gate, and the chunks are
// ANDed as before.  No gate reads an encrypted content block.  The program depends on
// (n_chars, m, lo, hi, starts) alone, never on the content bytes.
// bytes: the needle is a byte-table needle (keys.h), one table per character: a start's tests are
// the m terms (table i, position p + i, 0) -- one sum and one SIGN gate of offset 1 - 2 m for
// m <= 16, else balanced chunks of the m tests.
Program compile_needle_clear(size_t n_chars, size_t m, size_t lo, size_t hi, bool starts, bool bytes = false);

// A scan of a long clear text (fr_scan_clear*): a start's result depends only on the m bytes of
// its window, so the search runs once per distinct window and every start reads its class.
// window_classes takes the starts p of [lo, min(hi, n)): cls[p - lo] is the index of p's window
// among the distinct windows in order of first appearance (-1: p + m > n, the start does not fit),
// first[d] the start at which class d first appears, and text the compacted text
// window_0 | window_1 | .. | window_{D-1} (D m bytes, D = first.size()).  Windows are compared
// byte for byte; every byte value is valid.
struct WindowClasses {
    std::vector<int32_t> cls;
    std::vector<size_t> first;
    std::vector<uint8_t> text;
};
WindowClasses window_classes(const uint8_t* text, size_t n, size_t m, size_t lo, size_t hi);
// The class count a scan's plan is compiled for: D rounded up to a multiple of SCAN_BUCKET, the
// spare windows copies of window 0 (harmless in an OR, referenced by no start).  Two texts with
// nearby D share one cached plan at the price of at most SCAN_BUCKET - 1 spare rotations.
constexpr size_t SCAN_BUCKET = 64;
inline size_t scan_padded(size_t D) { return (D + SCAN_BUCKET - 1) / SCAN_BUCKET * SCAN_BUCKET; }
// wc.text grown to scan_padded(D) windows of m bytes: the text a scan's plan reads
void pad_window_text(WindowClasses& wc, size_t m);
// compile_needle_clear over a compacted text of n_windows windows of m bytes: start d reads the
// bytes from d m on (the clear layer at stride m), so window d's term t is (sel t, pos d m + t / 2,
// half t % 2); above the extract-sums the program is compile_needle_clear's for n_windows starts
// that all fit.  m = 1 is compile_needle_clear(n_windows, 1, 0, n_windows, starts) gate for gate.
// The program depends on (n_windows, m, starts) alone.  n_windows m <= 2^24.
// bytes: window d's term i is (table i, pos d m + i, 0), as compile_needle_clear's byte variant.
Program compile_needle_windows(size_t n_windows, size_t m, bool starts, bool bytes = false);
// What a match is over (match.cpp: the request), and the one place that maps a needle kind to its
// compile function above; windows: n its windows, [lo, hi) not used.
enum MatchKind : int { MATCH_PATTERN, MATCH_NEEDLE, MATCH_NEEDLE_CLEAR, MATCH_NEEDLE_WINDOWS };
// bytes: the needle's form; only the clear kinds have a byte variant (MATCH_NEEDLE refuses it).
Program needle_program(MatchKind kind, size_t n, size_t m, size_t lo, size_t hi, bool starts, bool bytes = false);

// LUT builders
void lut_eq(uint8_t* lut, int v);     // [x == v]
void lut_sign(uint8_t* lut, int v);   // x < v -> 0, x == v -> 1, x > v -> 2
void lut_gt3(uint8_t* lut, bool le);  // over 3*s_hi + s_lo: gt (or its negation)
void lut_at_least(uint8_t* lut, int m);

// Gate builders shared by the lowerings and the eager ops of the C ABI.
inline int cblk(int pos, int blk) { return -(1 + pos * 4 + blk); }
// a test of one nibble (half 0: low) of the character at pos, packed as x_{2h} + 4 x_{2h+1}:
// [nibble == v], or (sign) its comparison with v as lut_sign
PGate nibble_test_gate(bool sign, int pos, int half, int v);
// the last gate of a comparison with a constant, over its two nibble tests: equality
// [lo + hi == 2] over the eq tests, else gt (le: its negation) over 3 * sign_hi + sign_lo
PGate cmp_final_gate(VNode::Op op, int lo_gate, int hi_gate);
// the two-input gate of a faithful AND / OR: each operand a literal (gate, negated) or a
// constant (gate < 0: the value c); offset = 2 * (constants' values + negated literals)
struct PairOperand {
    int gate;  // < 0: the constant c
    bool neg;
    int c;
};
PGate pair_gate(bool is_and, const PairOperand& p, const PairOperand& q);
// m items cut into ceil(m / 16) contiguous chunks of near-equal length (the longer ones
// first): f(start, len) per chunk -- one level of a balanced threshold tree
template <class F>
void for_balanced_chunks(size_t m, F&& f) {
    const size_t chunks = (m + MAX_FANIN - 1) / MAX_FANIN;
    for (size_t c = 0, start = 0; c < chunks; ++c) {
        const size_t len = m / chunks + (c < m % chunks ? 1 : 0);
        f(start, len);
        start += len;
    }
}

}  // namespace fr
