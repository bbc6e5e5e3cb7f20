// extern "C" boundary (include/fheregex.h): context, keys, encryption, wire formats,
// ciphertext handles, eager gate ops (the smart_* replacements), plain evaluators and
// device hooks.  The executor is plan.cpp, the has_match engine match.cpp.
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "rns.h"
#include "step_sched.h"

using namespace fr;

namespace fr {

static thread_local std::string g_last_error;
void set_last_error(const std::string& m) { g_last_error = m; }

Params params_from_c(const fr_params* c) {
    Params p;
    if (c) {
        p.k = c->k;
        p.N = c->N;
        p.n = c->n;
        p.ks_base_log = c->ks_base_log;
        p.ks_level = c->ks_level;
        p.pbs_base_log = c->pbs_base_log;
        p.pbs_level = c->pbs_level;
        p.ring = c->ring;
        p.lwe_sigma = c->lwe_sigma;
        p.glwe_sigma = c->glwe_sigma;
    }
    validate_params(p);
    return p;
}
void validate_params(const Params& p) {
    if (p.k < 1 || p.k > 4 || p.N < 256 || p.N > 4096 || (p.N & (p.N - 1)) || p.n < 1 || p.n > 1024)
        throw Error(FR_ERR_INVALID, "invalid params");
    if (p.pbs_base_log != 23 || p.pbs_level != 1) throw Error(FR_ERR_INVALID, "only the 2^23 x 1 PBS gadget is supported");
    if (p.ks_base_log < 1 || p.ks_base_log * p.ks_level > 63) throw Error(FR_ERR_INVALID, "invalid keyswitch gadget");
    if (p.ring != FR_RING_RNS && p.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "invalid ring");
    if (p.ring == FR_RING_FFT && !((p.k == 1 && p.N == 2048) || (p.k == 2 && p.N == 1024)))
        throw Error(FR_ERR_INVALID, "the FFT ring is built for (k, N) = (1, 2048) and (2, 1024)");
}

}  // namespace fr

// eager op programs over input handles (pos 0 = a, pos 1 = b)
// one output: the program's last gate
static Program one_output(std::vector<PGate>&& gates) {
    Program p;
    p.gates = std::move(gates);
    p.outs.push_back(ProgOut{(int32_t)p.gates.size() - 1, 1, 0});
    compute_levels(p);
    return p;
}
// the lowering's comparison gates: the low and the high nibble test, then their combination
static Program prog_cmp_const(VNode::Op op, uint8_t c) {
    const bool sign = op != VNode::EQ;
    return one_output({nibble_test_gate(sign, 0, 0, c & 15), nibble_test_gate(sign, 0, 1, c >> 4), cmp_final_gate(op, 0, 1)});
}

extern "C" {

const char* fr_last_error(void) { return fr::g_last_error.c_str(); }

int fr_default_params(fr_params* out) {
    FR_TRY({
        NEED(out);
        Params p;
        std::memset(out, 0, sizeof *out);
        out->k = p.k;
        out->N = p.N;
        out->n = p.n;
        out->ks_base_log = p.ks_base_log;
        out->ks_level = p.ks_level;
        out->pbs_base_log = p.pbs_base_log;
        out->pbs_level = p.pbs_level;
        out->ring = p.ring;
        out->lwe_sigma = p.lwe_sigma;
        out->glwe_sigma = p.glwe_sigma;
    })
}

int fr_ctx_create(const fr_params* params, int device, fr_ctx** out) {
    FR_TRY({
        NEED(out);
        *out = nullptr;
        auto ctx = std::make_unique<fr_ctx>();
        ctx->p = params_from_c(params);
        if (device >= 0) ctx->dev = std::make_unique<Device>(ctx->p, device);
        *out = ctx.release();
    })
}

int fr_ctx_destroy(fr_ctx* ctx) {
    FR_TRY({ delete ctx; })
}

int fr_set_lowering(fr_ctx* ctx, int32_t mode) {
    FR_TRY({
        NEED(ctx && (mode == FR_LOWER_FAITHFUL || mode == FR_LOWER_THRESHOLD || mode == FR_LOWER_FAITHFUL_TREE));
        ctx->lowering = mode;
    })
}

int fr_set_engine(fr_ctx* ctx, int32_t engine) {
    FR_TRY({
        NEED(ctx && engine >= FR_ENGINE_AUTO && engine <= FR_ENGINE_MERGED);
        ctx->engine = engine;
    })
}

int fr_set_keygen(fr_ctx* ctx, int32_t where) {
    FR_TRY({
        NEED(ctx && where >= FR_KEYGEN_AUTO && where <= FR_KEYGEN_DEVICE);
        ctx->keygen = where;
    })
}

int fr_set_grammar(fr_ctx* ctx, int32_t grammar) {
    FR_TRY({
        NEED(ctx && (grammar == FR_GRAMMAR_REFERENCE || grammar == FR_GRAMMAR_EXT));
        ctx->grammar = grammar;
    })
}

int fr_set_multi_value(fr_ctx* ctx, int32_t on) {
    FR_TRY({
        NEED(ctx);
        ctx->multi_value = on != 0;
    })
}

int fr_dev_blind_rotate_multi(fr_ctx* ctx, const uint64_t* in, const uint8_t* luts, int32_t n_out, int32_t direct,
                              uint64_t* out) {
    FR_TRY({
        NEED(ctx && in && luts && out);
        ctx->device().blind_rotate_multi_host(in, luts, n_out, direct, out);
    })
}

int fr_set_profiling(fr_ctx* ctx, int32_t on) {
    FR_TRY({
        NEED(ctx && on >= 0 && on <= 2);  // 0 off, 1 blind-rotation timers, 2 the keyswitch timers too
        ctx->device().set_profiling(on);
    })
}

int fr_device_info(fr_ctx* ctx, char* buf, size_t len) {
    FR_TRY({
        NEED(ctx && buf && len);
        std::string s = ctx->dev ? ctx->dev->info() : std::string("host-only");
        std::snprintf(buf, len, "%s", s.c_str());
    })
}

int fr_upload_radix(fr_ctx* ctx, const uint64_t* blocks, size_t n, fr_ct* out) {
    FR_TRY({
        NEED(ctx && (blocks || !n) && (out || !n));
        Device& dev = ctx->device();
        Slots slots(dev, 4 * n);
        dev.write_slots(slots.data(), slots.size(), blocks);
        ctx->adopt(std::move(slots), true, out);
    })
}

int fr_upload_bool(fr_ctx* ctx, const uint64_t* lwe, size_t n, fr_ct* out) {
    FR_TRY({
        NEED(ctx && (lwe || !n) && (out || !n));
        Device& dev = ctx->device();
        Slots slots(dev, n);
        dev.write_slots(slots.data(), n, lwe);
        ctx->adopt(std::move(slots), false, out);
    })
}

int fr_download_radix(fr_ctx* ctx, fr_ct h, uint64_t* out) {
    FR_TRY({
        NEED(ctx && out);
        HandleRec& r = ctx->get(h);
        const int L = ctx->p.lwe_len();
        for (int b = 0; b < 4; ++b) {
            uint64_t* o = out + (size_t)b * L;
            if (r.b[b].slot >= 0) {
                ctx->device().read_slot(r.b[b].slot, o);
            } else {  // trivial block (shortint create_trivial): zero mask, body m * Delta
                std::memset(o, 0, 8 * (size_t)L);
                o[L - 1] = (uint64_t)r.b[b].triv << DELTA_LOG;
            }
        }
    })
}

int fr_release(fr_ctx* ctx, fr_ct h) {
    FR_TRY({
        NEED(ctx);
        ctx->release(h);
    })
}

int fr_trivial(fr_ctx* ctx, uint8_t value, fr_ct* out) {
    FR_TRY({  // create_trivial_radix, ciphertext.rs:8-30
        NEED(ctx && out);
        HandleRec r;
        for (int b = 0; b < 4; ++b) r.b[b].triv = (value >> (2 * b)) & 3;
        *out = ctx->new_handle(r);
    })
}

static int cmp_const_op(fr_ctx* ctx, fr_ct a, uint8_t c, fr_ct* out, VNode::Op op) {
    FR_TRY({
        NEED(ctx && out);
        if (ctx->get(a).is_bool) throw Error(FR_ERR_INVALID, "comparison operand must be a radix character");
        Program p = prog_cmp_const(op, c);
        *out = run_program(ctx, p, {a}, nullptr);
    })
}
int fr_eq_const(fr_ctx* ctx, fr_ct a, uint8_t c, fr_ct* out) { return cmp_const_op(ctx, a, c, out, VNode::EQ); }
int fr_gt_const(fr_ctx* ctx, fr_ct a, uint8_t c, fr_ct* out) { return cmp_const_op(ctx, a, c, out, VNode::GT); }
int fr_le_const(fr_ctx* ctx, fr_ct a, uint8_t c, fr_ct* out) { return cmp_const_op(ctx, a, c, out, VNode::LE); }

static int bitop(fr_ctx* ctx, fr_ct a, fr_ct b, fr_ct* out, bool is_and) {
    FR_TRY({
        NEED(ctx && out);
        const HandleRec& ha = ctx->get(a);
        const HandleRec& hb = ctx->get(b);
        if (ha.is_bool && hb.is_bool) {  // booleans: one bivariate PBS on block 0
            PGate g;
            g.ins = {{cblk(0, 0), 1}, {cblk(1, 0), 1}};
            if (is_and) lut_eq(g.lut, 2);
            else lut_at_least(g.lut, 1);
            const Program p = one_output({g});
            *out = run_program(ctx, p, {a, b}, nullptr);
        } else {  // general radix: per block, LUT over 4*x + y
            std::vector<PGate> gates(4);
            for (int blk = 0; blk < 4; ++blk) {
                gates[blk].ins = {{cblk(0, blk), 4}, {cblk(1, blk), 1}};
                for (int v = 0; v < 16; ++v) gates[blk].lut[v] = (uint8_t)(is_and ? ((v >> 2) & (v & 3)) : ((v >> 2) | (v & 3)));
            }
            Slots slots = execute_gates(ctx, gates, {a, b}, nullptr);
            ctx->device().sync();
            ctx->adopt(std::move(slots), true, out);
        }
    })
}
int fr_and(fr_ctx* ctx, fr_ct a, fr_ct b, fr_ct* out) { return bitop(ctx, a, b, out, true); }
int fr_or(fr_ctx* ctx, fr_ct a, fr_ct b, fr_ct* out) { return bitop(ctx, a, b, out, false); }

int fr_not(fr_ctx* ctx, fr_ct a, fr_ct* out) {
    FR_TRY({  // smart_bitxor(a, trivial 1), execution.rs:178-195
        NEED(ctx && out);
        const HandleRec ha = ctx->get(a);
        if (ha.is_bool) {
            if (ha.b[0].slot < 0) {
                *out = ctx->new_bool(-1, ha.b[0].triv ^ 1);
            } else {  // 1 - a
                Slots s = linear_to_new_slot(ctx->device(), ha.b[0].slot, -1, 2);
                ctx->device().sync();
                ctx->adopt(std::move(s), false, out);
            }
        } else {  // general radix: block 0 through a LUT, blocks 1..3 copied
            std::vector<PGate> gates(1);
            gates[0].ins = {{cblk(0, 0), 1}};
            for (int v = 0; v < 16; ++v) gates[0].lut[v] = (uint8_t)((v & 3) ^ 1);
            Slots part[4];  // one slot each; a trivial block has none
            part[0] = execute_gates(ctx, gates, {a}, nullptr);
            for (int blk = 1; blk < 4; ++blk)
                if (ha.b[blk].slot >= 0) part[blk] = linear_to_new_slot(ctx->device(), ha.b[blk].slot, 1, 0);
            ctx->device().sync();
            ctx->reserve_handles(1);  // new_handle cannot fail once the slots have left their owners
            HandleRec r;
            for (int blk = 0; blk < 4; ++blk) {
                if (part[blk].size()) r.b[blk].slot = part[blk].take(0);
                else r.b[blk] = ha.b[blk];
            }
            *out = ctx->new_handle(r);
        }
    })
}

int fr_or_many(fr_ctx* ctx, const fr_ct* in, size_t n, fr_ct* out) {
    FR_TRY({
        NEED(ctx && out && (in || !n));
        std::vector<fr_ct> inputs;
        int triv_or = 0;
        for (size_t i = 0; i < n; ++i) {
            const HandleRec& h = ctx->get(in[i]);
            if (!h.is_bool) throw Error(FR_ERR_INVALID, "fr_or_many: inputs must be booleans");
            if (h.b[0].slot < 0) triv_or |= h.b[0].triv & 1;
            else inputs.push_back(in[i]);
        }
        if (triv_or || inputs.empty()) {
            *out = ctx->new_bool(-1, (uint8_t)triv_or);
            return FR_OK;
        }
        if (inputs.size() == 1) {  // copy
            Slots s = linear_to_new_slot(ctx->device(), ctx->get(inputs[0]).b[0].slot, 1, 0);
            ctx->device().sync();
            ctx->adopt(std::move(s), false, out);
            return FR_OK;
        }
        // balanced tree of <= 16-input threshold ORs
        std::vector<PGate> gates;
        std::vector<int> cur;  // sources: negative = input q, else gate
        for (size_t q = 0; q < inputs.size(); ++q) cur.push_back(cblk((int)q, 0));
        while (cur.size() > 1) {
            std::vector<int> next;
            for_balanced_chunks(cur.size(), [&](size_t start, size_t len) {
                if (len == 1) {
                    next.push_back(cur[start]);
                    return;
                }
                PGate g;  // OR of <= 16 booleans: sign of sum - 1/2
                for (size_t t = 0; t < len; ++t) g.ins.push_back({cur[start + t], 1});
                g.kind = GATE_SIGN;
                g.offset = -1;
                gates.push_back(g);
                next.push_back((int)gates.size() - 1);
            });
            cur = next;
        }
        *out = run_program(ctx, one_output(std::move(gates)), inputs, nullptr);
    })
}

int fr_run_gates(fr_ctx* ctx, fr_gate* gates, size_t n) {
    FR_TRY({
        NEED(ctx && (gates || !n));
        std::vector<fr_ct> inputs;
        std::vector<std::pair<fr_ct, int>> seen;
        auto input_index = [&](fr_ct h) -> int {
            for (size_t i = 0; i < inputs.size(); ++i)
                if (inputs[i] == h) return (int)i;
            ctx->get(h);
            inputs.push_back(h);
            return (int)inputs.size() - 1;
        };
        std::vector<PGate> pg(n);
        for (size_t j = 0; j < n; ++j) {
            const fr_gate& g = gates[j];
            NEED(g.n_in >= 0 && g.n_in <= 16 && (g.kind == GATE_LUT || g.kind == GATE_SIGN));
            pg[j].offset = g.offset;
            pg[j].kind = g.kind;
            std::memcpy(pg[j].lut, g.lut, 16);
            for (int q = 0; q < g.n_in; ++q) {
                if (g.in[q] & 0x80000000u) {
                    uint32_t src = g.in[q] & 0x7FFFFFFFu;
                    NEED(src < j);
                    pg[j].ins.push_back({(int)src, g.in_w[q]});
                } else {
                    NEED(g.in_block[q] >= 0 && g.in_block[q] < 4);
                    pg[j].ins.push_back({cblk(input_index(g.in[q]), g.in_block[q]), g.in_w[q]});
                }
            }
        }
        Slots slots = execute_gates(ctx, pg, inputs, nullptr);
        ctx->device().sync();
        std::vector<fr_ct> outs(n);
        ctx->adopt(std::move(slots), false, outs.data());
        for (size_t j = 0; j < n; ++j) gates[j].out = outs[j];
    })
}

int fr_debug_enumeration_cost(const char* pattern, int32_t grammar, size_t n_chars, size_t lo, size_t hi,
                              uint64_t cap, uint64_t mem_bytes, int32_t enumerate, int32_t* outcome,
                              uint64_t* counted, uint64_t* enumerated) {
    FR_TRY({
        NEED(pattern && outcome && counted && enumerated && lo <= hi && cap < UINT64_MAX);
        NEED(grammar == FR_GRAMMAR_REFERENCE || grammar == FR_GRAMMAR_EXT);
        ReP re = parse(pattern, grammar);
        uint64_t c = 0;
        const CostOutcome o = enumeration_cost(n_chars, re, lo, hi, cap, &c, mem_bytes);
        *outcome = o == COST_COUNTED ? FR_COST_COUNTED : o == COST_PANIC ? FR_COST_PANIC : FR_COST_MEMORY;
        *counted = o == COST_COUNTED ? c : 0;
        *enumerated = enumerate ? enumeration_spent(n_chars, re, lo, hi, cap) : 0;
    })
}

// the recorded circuit and its lowered program on a plaintext content; vals: each part's value
static void plain_match(const char* content, size_t len, const char* pattern, size_t lo, size_t hi, int32_t lowering,
                        int32_t engine, int32_t grammar, size_t max_parts, fr_plain_result* out,
                        std::vector<int>& vals) {
    std::memset(out, 0, sizeof *out);
    const CompiledMatch cm = compile_match(MatchSpec{pattern, len, lo, hi, engine, grammar, lowering, (int)max_parts});
    const Recorded& rec = cm.rec;
    const Program& prog = cm.prog;
    std::vector<int16_t> memo;
    out->ct_ops = rec.ct_ops;
    out->cache_hits = rec.cache_hits;
    out->n_branches = rec.n_branches;
    out->result_recorded = cm.dag.eval(rec.root, (const uint8_t*)content, memo);
    out->pbs = prog.gates.size();
    out->levels = (uint64_t)prog.levels;
    out->max_level_width = prog.max_width;
    out->result_lowered = eval_program_parts(prog, (const uint8_t*)content, len, vals);
}

int fr_plain_match_parts(const char* content, size_t len, const char* pattern, size_t lo, size_t hi, int32_t lowering,
                         int32_t engine, int32_t grammar, size_t max_parts, fr_plain_result* out, int32_t* parts,
                         size_t* n_parts) {
    FR_TRY({
        NEED((content || !len) && pattern && out && parts && n_parts && lo <= hi);
        NEED(max_parts >= 1 && max_parts <= (size_t)MAX_FANIN);
        NEED(lowering >= FR_LOWER_FAITHFUL && lowering <= FR_LOWER_FAITHFUL_TREE);
        NEED(engine >= FR_ENGINE_AUTO && engine <= FR_ENGINE_MERGED);
        NEED(grammar == FR_GRAMMAR_REFERENCE || grammar == FR_GRAMMAR_EXT);
        std::vector<int> vals;
        plain_match(content, len, pattern, lo, hi, lowering, engine, grammar, max_parts, out, vals);
        for (size_t j = 0; j < vals.size(); ++j) parts[j] = vals[j];
        *n_parts = vals.size();
    })
}

int fr_plain_match_starts(const char* content, size_t len, const char* pattern, size_t lo, size_t hi, int32_t lowering,
                          int32_t engine, int32_t grammar, fr_plain_result* out, int32_t* lowered,
                          int32_t* recorded, size_t cap, size_t* n_starts) {
    FR_TRY({
        NEED((content || !len) && pattern && out && n_starts && lo <= hi && cap >= hi - lo);
        NEED((lowered && recorded) || lo == hi);
        NEED(lowering >= FR_LOWER_FAITHFUL && lowering <= FR_LOWER_FAITHFUL_TREE);
        NEED(engine >= FR_ENGINE_AUTO && engine <= FR_ENGINE_MERGED);
        NEED(grammar == FR_GRAMMAR_REFERENCE || grammar == FR_GRAMMAR_EXT);
        std::memset(out, 0, sizeof *out);
        const CompiledStarts cs =
            compile_match_starts(MatchSpec{pattern, len, lo, hi, engine, grammar, lowering, 1}, true);
        std::vector<int> vals;
        out->result_lowered = eval_program_parts(cs.prog, (const uint8_t*)content, len, vals);
        out->ct_ops = cs.rec.ct_ops;
        out->cache_hits = cs.rec.cache_hits;
        out->n_branches = cs.rec.n_branches;
        out->pbs = cs.prog.gates.size();
        out->levels = (uint64_t)cs.prog.levels;
        out->max_level_width = cs.prog.max_width;
        for (size_t j = 0; j < vals.size(); ++j) {
            std::vector<int16_t> memo;
            lowered[j] = vals[j];
            recorded[j] = cs.dags[j].eval(cs.roots[j], (const uint8_t*)content, memo);
            out->result_recorded |= recorded[j];
        }
        *n_starts = vals.size();
    })
}

int fr_parse(const char* pattern, char* buf, size_t len) {
    return fr_parse_ex(pattern, FR_GRAMMAR_REFERENCE, buf, len);
}

int fr_parse_ex(const char* pattern, int32_t grammar, char* buf, size_t len) {
    FR_TRY({
        NEED(pattern && buf && len);
        std::string s = to_string(*parse(pattern, grammar));
        if (s.size() + 1 > len) throw Error(FR_ERR_INVALID, "buffer too small");
        std::memcpy(buf, s.c_str(), s.size() + 1);
    })
}

int fr_plain_match_ex(const char* content, size_t len, const char* pattern, size_t lo, size_t hi, int32_t lowering,
                      int32_t engine, fr_plain_result* out) {
    return fr_plain_match_g(content, len, pattern, lo, hi, lowering, engine, FR_GRAMMAR_REFERENCE, out);
}

int fr_plain_match_g(const char* content, size_t len, const char* pattern, size_t lo, size_t hi, int32_t lowering,
                     int32_t engine, int32_t grammar, fr_plain_result* out) {
    FR_TRY({
        NEED((content || !len) && pattern && out && lo <= hi);
        NEED(engine >= FR_ENGINE_AUTO && engine <= FR_ENGINE_MERGED);
        NEED(grammar == FR_GRAMMAR_REFERENCE || grammar == FR_GRAMMAR_EXT);
        std::vector<int> vals;  // one part (the lowering decides whether `lowering` is valid)
        plain_match(content, len, pattern, lo, hi, lowering, engine, grammar, 1, out, vals);
    })
}

int fr_plain_match(const char* content, size_t len, const char* pattern, size_t lo, size_t hi, int32_t lowering,
                   fr_plain_result* out) {
    return fr_plain_match_ex(content, len, pattern, lo, hi, lowering, FR_ENGINE_ENUMERATE, out);
}

int fr_dev_keyswitch(fr_ctx* ctx, const uint64_t* in, size_t count, uint64_t* out) {
    FR_TRY({
        NEED(ctx && in && out);
        ctx->device().keyswitch_host(in, count, out);
    })
}
int fr_dev_blind_rotate(fr_ctx* ctx, const uint64_t* in, const uint8_t* luts, size_t count, uint64_t* out) {
    FR_TRY({
        NEED(ctx && in && luts && out);
        ctx->device().blind_rotate_host(in, luts, count, out);
    })
}
int fr_dev_blind_rotate_acc(fr_ctx* ctx, const uint64_t* in, const uint64_t* accs, size_t count, uint64_t* out) {
    FR_TRY({
        NEED(ctx && in && accs && out);
        ctx->device().blind_rotate_acc_host(in, accs, count, out);
    })
}
// A needle search on a plaintext, both lowered programs gate by gate: the per-start values from
// the starts program, `any` from the boolean program's OR tree.  cls (a scan): start j reads the
// output of its class (none, or past the classed starts: 0); else start j reads output j.
// byte_tables: a byte-table needle's m sets of 256 bits instead of the 2 m masks.
static void plain_needle(MatchKind kind, const uint8_t* text, size_t len, size_t n, size_t m, size_t lo, size_t hi,
                         const uint16_t* masks, const std::vector<int32_t>* cls, uint8_t* starts_out, int32_t* any,
                         const uint8_t* byte_tables = nullptr) {
    std::vector<int> vals;
    const bool bytes = byte_tables != nullptr;
    const size_t n_tables = bytes ? m : 2 * m;
    eval_program_parts(needle_program(kind, n, m, lo, hi, true, bytes), text, len, vals, masks, n_tables, byte_tables);
    for (size_t j = 0; j < (cls ? hi - lo : vals.size()); ++j) {
        const long o = !cls ? (long)j : j < cls->size() ? (*cls)[j] : -1;
        starts_out[j] = o >= 0 ? (uint8_t)vals[(size_t)o] : 0;
    }
    *any = eval_program_parts(needle_program(kind, n, m, lo, hi, false, bytes), text, len, vals, masks, n_tables,
                              byte_tables);
}
int fr_plain_find(const char* content, size_t len, const uint16_t* masks, size_t m, size_t start_lo, size_t start_hi,
                  uint8_t* starts_out, int32_t* any) {
    FR_TRY({
        NEED((content || !len) && masks && any && start_lo <= start_hi && (starts_out || start_lo == start_hi));
        NEED(m >= 1 && m <= NEEDLE_MAX_CHARS);
        plain_needle(MATCH_NEEDLE, (const uint8_t*)content, len, len, m, start_lo, start_hi, masks, nullptr, starts_out,
                     any);
    })
}
int fr_plain_find_clear(const uint8_t* content, size_t len, const uint16_t* masks, size_t m, size_t start_lo,
                        size_t start_hi, uint8_t* starts_out, int32_t* any) {
    FR_TRY({
        NEED((content || !len) && masks && any && start_lo <= start_hi && (starts_out || start_lo == start_hi));
        NEED(m >= 1 && m <= NEEDLE_MAX_CHARS);
        plain_needle(MATCH_NEEDLE_CLEAR, content, len, len, m, start_lo, start_hi, masks, nullptr, starts_out, any);
    })
}
int fr_window_classes(const uint8_t* text, size_t n_chars, size_t m, size_t start_lo, size_t start_hi, int32_t* cls,
                      size_t cls_cap, size_t* n_cls, uint64_t* classes, uint64_t* padded, uint8_t* windows,
                      size_t windows_cap) {
    FR_TRY({
        NEED((text || !n_chars) && n_cls && classes && padded && start_lo <= start_hi);
        const WindowClasses wc = window_classes(text, n_chars, m, start_lo, start_hi);
        *n_cls = wc.cls.size();
        *classes = wc.first.size();
        *padded = scan_padded(wc.first.size());
        if (cls) {
            NEED(cls_cap >= wc.cls.size());
            std::copy(wc.cls.begin(), wc.cls.end(), cls);
        }
        if (windows) {
            NEED(windows_cap >= wc.text.size());
            std::copy(wc.text.begin(), wc.text.end(), windows);
        }
    })
}
int fr_plain_scan_clear(const uint8_t* content, size_t len, const uint16_t* masks, size_t m, size_t start_lo,
                        size_t start_hi, uint8_t* starts_out, int32_t* any) {
    FR_TRY({
        NEED((content || !len) && masks && any && start_lo <= start_hi && (starts_out || start_lo == start_hi));
        NEED(m >= 1 && m <= NEEDLE_MAX_CHARS && start_hi - start_lo <= ((size_t)1 << 24));
        // the scan's own route: class the windows, then the programs over the padded compacted text
        WindowClasses wc = window_classes(content, len, m, start_lo, start_hi);
        pad_window_text(wc, m);
        plain_needle(MATCH_NEEDLE_WINDOWS, wc.text.data(), wc.text.size(), scan_padded(wc.first.size()), m, start_lo,
                     start_hi, masks, &wc.cls, starts_out, any);
    })
}
int fr_plain_find_clear_bytes(const uint8_t* content, size_t len, const uint8_t* tables, size_t m, size_t start_lo,
                              size_t start_hi, uint8_t* starts_out, int32_t* any) {
    FR_TRY({
        NEED((content || !len) && tables && any && start_lo <= start_hi && (starts_out || start_lo == start_hi));
        NEED(m >= 1 && m <= NEEDLE_MAX_CHARS);
        plain_needle(MATCH_NEEDLE_CLEAR, content, len, len, m, start_lo, start_hi, nullptr, nullptr, starts_out, any,
                     tables);
    })
}
int fr_plain_scan_clear_bytes(const uint8_t* content, size_t len, const uint8_t* tables, size_t m, size_t start_lo,
                              size_t start_hi, uint8_t* starts_out, int32_t* any) {
    FR_TRY({
        NEED((content || !len) && tables && any && start_lo <= start_hi && (starts_out || start_lo == start_hi));
        NEED(m >= 1 && m <= NEEDLE_MAX_CHARS && start_hi - start_lo <= ((size_t)1 << 24));
        WindowClasses wc = window_classes(content, len, m, start_lo, start_hi);
        pad_window_text(wc, m);
        plain_needle(MATCH_NEEDLE_WINDOWS, wc.text.data(), wc.text.size(), scan_padded(wc.first.size()), m, start_lo,
                     start_hi, nullptr, &wc.cls, starts_out, any, tables);
    })
}
int fr_dev_select_sum(fr_ctx* ctx, const fr_needle* needle, const uint8_t* content, size_t len, const int32_t* terms,
                      const int32_t* n_terms, size_t n_sums, uint64_t* out) {
    FR_TRY({
        NEED(ctx && needle && (content || !len) && terms && n_terms && out);
        Device& dev = ctx->device();
        if (needle->k != ctx->p.k || needle->N != ctx->p.N)
            throw Error(FR_ERR_INVALID, "needle: k, N do not match the context params");
        dev.select_sum_host(needle->dev, content, len, terms, n_terms, n_sums, out);
    })
}
int fr_dev_select_sum_ms(fr_ctx* ctx, double* ms) {
    FR_TRY({
        NEED(ctx && ms);
        *ms = ctx->device().select_sum_ms();
    })
}
int fr_dev_ring_mul(fr_ctx* ctx, const uint64_t* a, const uint64_t* b, size_t count, uint64_t* out) {
    FR_TRY({
        NEED(ctx && a && b && out);
        ctx->device().ring_mul_host(a, b, count, out);
    })
}
int fr_dev_bench_pbs(fr_ctx* ctx, const fr_ct* in, size_t count, int32_t iters, double* br_ms, double* total_ms) {
    FR_TRY({
        NEED(ctx && in && count && iters > 0 && br_ms && total_ms);
        Device& dev = ctx->device();
        if (!ctx->has_sk) throw Error(FR_ERR_NO_KEY, "server key not generated");
        std::vector<DevGate> gates(count);
        for (size_t i = 0; i < count; ++i) {
            const HandleRec& h = ctx->get(in[i]);
            DevGate& d = gates[i];
            std::memset(&d, 0, sizeof d);
            int nin = 0, off = 0;
            // pack x0 + 4*x1 of a radix char (or a boolean's block 0): an eq-nibble PBS
            const int w[2] = {1, 4};
            for (int b = 0; b < (h.is_bool ? 1 : 2); ++b) {
                if (h.b[b].slot < 0) {
                    off += w[b] * h.b[b].triv;
                    continue;
                }
                d.in_slot[nin] = h.b[b].slot;
                d.in_w[nin] = w[b];
                ++nin;
            }
            d.n_in = nin;
            d.offset = 2 * off;
            lut_eq(d.lut[0], 1);
            d.n_out = 1;
            d.direct = JOB_DIRECT;
        }
        Slots outs(dev, count);  // once every handle has been checked
        for (size_t i = 0; i < count; ++i) gates[i].out_slot[0] = outs[i];
        dev.bench_pbs(gates, iters, br_ms, total_ms);
    })
}

uint64_t fr_debug_scalar(int32_t op, uint64_t x, uint64_t y) {
    switch (op) {
        case 0: return rns::crt((uint32_t)(x % rns::P0), (uint32_t)(x % rns::P1));
        case 1: return (uint64_t)(int64_t)rns::decompose((uint32_t)(x % rns::P0), (uint32_t)(x % rns::P1));
        case 2: return rns::to_torus((uint32_t)(x % rns::P0), (uint32_t)(x % rns::P1));
        case 3: return mod_switch(x, (int)y);
        case 4: {
            int32_t d[5];
            ks_decompose<3, 5>(x, d);
            return (uint64_t)(int64_t)d[y % 5];
        }
        case 5: return step_sched::put(x, (int)((y >> step_sched::FIELD_BITS) % step_sched::FIELDS), (uint32_t)y);
        case 6: return step_sched::get(x, (int)(y % step_sched::FIELDS));
        default: return 0;
    }
}

int fr_debug_arena_stats(fr_ctx* ctx, uint64_t* slots, uint64_t* free_slots) {
    FR_TRY({
        NEED(ctx && slots && free_slots);
        Device& dev = ctx->device();
        dev.sync();  // every lane: the deferred frees return to the free list
        *slots = dev.arena_slots();
        *free_slots = dev.arena_free_slots();
    })
}

int fr_debug_handle_count(fr_ctx* ctx, uint64_t* live) {
    FR_TRY({
        NEED(ctx && live);
        *live = ctx->handles.size() - ctx->free_handles.size();
    })
}

// device-to-device booleans (block 0 of a handle), e.g. per-rank partial results
// gathered over RCCL: no host round trip of the LWE
int fr_export_bool_device(fr_ctx* ctx, const fr_ct* h, size_t n, uint64_t* dev_dst) {
    FR_TRY({
        NEED(ctx && (h || !n) && (dev_dst || !n));
        Device& dev = ctx->device();
        std::vector<int> slots(n);
        size_t n_triv = 0;
        for (size_t i = 0; i < n; ++i) {
            slots[i] = ctx->get(h[i]).b[0].slot;
            n_triv += slots[i] < 0;
        }
        // a trivial block 0 (e.g. a start range that cannot match): its trivial LWE in a slot
        // of the call's own
        Slots tmp(dev, n_triv);
        std::vector<uint64_t> lwe((size_t)ctx->p.lwe_len(), 0);
        for (size_t i = 0, t = 0; i < n; ++i) {
            if (slots[i] >= 0) continue;
            lwe.back() = (uint64_t)ctx->get(h[i]).b[0].triv << DELTA_LOG;
            slots[i] = tmp[t++];
            dev.write_slots(&slots[i], 1, lwe.data());
        }
        dev.slots_to_device(slots.data(), n, dev_dst);
    })
}
int fr_export_bool_device_async(fr_ctx* ctx, const fr_ct* h, size_t n, uint64_t* dev_dst) {
    FR_TRY({
        NEED(ctx && (h || !n) && (dev_dst || !n));
        if (n > 16) throw Error(FR_ERR_INVALID, "fr_export_bool_device_async: at most 16 handles");
        std::vector<int> slots(n);
        for (size_t i = 0; i < n; ++i) {
            const HandleRec& r = ctx->get(h[i]);
            if (r.b[0].slot < 0) return fr_export_bool_device(ctx, h, n, dev_dst);  // trivial: synchronising path
            slots[i] = r.b[0].slot;
        }
        ctx->device().slots_to_device_async(slots.data(), n, dev_dst);
    })
}
int fr_stream(fr_ctx* ctx, void** stream) {
    FR_TRY({
        NEED(ctx && stream);
        *stream = ctx->device().stream();
    })
}
int fr_import_bool_device(fr_ctx* ctx, const uint64_t* dev_src, size_t n, fr_ct* out) {
    FR_TRY({
        NEED(ctx && out && (dev_src || !n));
        Device& dev = ctx->device();
        Slots slots(dev, n);
        dev.device_to_slots(slots.data(), n, dev_src);
        ctx->adopt(std::move(slots), false, out);
    })
}
// the accumulated timers after a synchronise: one blind-rotation triple of them, and the keyswitch's
static int device_timers(fr_ctx* ctx, double DeviceTimers::*ms, uint64_t DeviceTimers::*launches,
                         uint64_t DeviceTimers::*gates, double* br_ms, double* ks_ms, uint64_t* br_launches,
                         uint64_t* br_gates) {
    FR_TRY({
        NEED(ctx);
        Device& dev = ctx->device();
        dev.sync();
        const DeviceTimers& t = dev.timers();
        if (br_ms) *br_ms = t.*ms;
        if (ks_ms) *ks_ms = t.ks_ms;
        if (br_launches) *br_launches = t.*launches;
        if (br_gates) *br_gates = t.*gates;
    })
}
int fr_device_timers_latency(fr_ctx* ctx, double* br_ms, uint64_t* br_launches, uint64_t* br_gates) {
    return device_timers(ctx, &DeviceTimers::lat_br_ms, &DeviceTimers::lat_launches, &DeviceTimers::lat_gates, br_ms,
                         nullptr, br_launches, br_gates);
}
int fr_device_timers_pair(fr_ctx* ctx, double* br_ms, uint64_t* br_launches, uint64_t* br_gates) {
    return device_timers(ctx, &DeviceTimers::pair_br_ms, &DeviceTimers::pair_launches, &DeviceTimers::pair_gates, br_ms,
                         nullptr, br_launches, br_gates);
}
int fr_device_timers_key_load(fr_ctx* ctx, double* ms) {
    FR_TRY({
        NEED(ctx && ms);
        std::memcpy(ms, ctx->device().key_load_ms(), 5 * sizeof(double));
    })
}
int fr_device_timers_packing_key_load(fr_ctx* ctx, double* ms) {
    FR_TRY({
        NEED(ctx && ms);
        std::memcpy(ms, ctx->device().pk_load_ms(), 3 * sizeof(double));
    })
}
int fr_device_timers_content(fr_ctx* ctx, double* ms) {
    FR_TRY({
        NEED(ctx && ms);
        *ms = ctx->device().expand_ms();
    })
}
int fr_device_timers(fr_ctx* ctx, double* br_ms, double* ks_ms, uint64_t* br_launches, uint64_t* br_gates) {
    return device_timers(ctx, &DeviceTimers::br_ms, &DeviceTimers::br_launches, &DeviceTimers::br_gates, br_ms, ks_ms,
                         br_launches, br_gates);
}

}  // extern "C"
