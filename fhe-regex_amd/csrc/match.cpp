// The match engine behind the C ABI: one request through three stages (the plan, by way of the
// plan cache; the launch; the reply) for has_match and its batch / range / parts / starts forms and
// the private searches, then the level-sharded match and the host-only schedule.
#include <climits>
#include <variant>

#include "ctx.h"

using namespace fr;

namespace {

// ------------------------------------------------------------ the request
// One match as the engine sees it: what is matched and where the result goes.  Every entry of
// fr_has_match*, fr_match_starts*, fr_find*, fr_find_clear* and fr_scan_clear* fills one and
// makes one call (run_match); validate states which combinations are legal.
// Handles: outs[m * P + j] for the P outputs of match m, P into *n_parts if asked for.
struct ToHandles {
    fr_ct* outs;
    size_t* n_parts;
};
// One packed blob of the starts (compact: FRCPRES1, else FRPKRES1), with no handle in between:
// packed_compact_size / packed_result_size bytes at buf.
struct ToBlob {
    bool compact;
    uint8_t* buf;
};
// A scan's reply: the plan's outputs are window classes and start j of the call's n_starts reads
// output cls[j] (-1: the constant 0); buf receives one blob per chunk of N starts, back to back
// (scan_reply_size bytes).
struct ToScanBlobs {
    bool compact;
    uint8_t* buf;
    const int32_t* cls;
    size_t n_starts;
};
using Sink = std::variant<ToHandles, ToBlob, ToScanBlobs>;
struct MatchRequest {
    // pattern: `pattern` over content handles.  The needle kinds (fr_find*: no pattern) match the
    // needle's encrypted tables, bound to the match's lane around its launches: over content
    // handles (compile_needle), over the n clear bytes at `text` (compile_needle_clear), or over a
    // clear text compacted to its n distinct windows, padded (compile_needle_windows over [0, n)).
    MatchKind kind = MATCH_PATTERN;
    bool starts = false;  // one boolean per start offset of [lo, hi) instead of their OR
    const char* pattern = "";
    // M independent matches over M contents of n positions each, content[m * n + q], in one plan;
    // parts > 1: each match returns up to `parts` booleans whose OR is its result
    const fr_ct* content = nullptr;
    size_t n = 0, M = 1, lo = 0, hi = 0, parts = 1;
    const fr_needle* needle = nullptr;
    const uint8_t* text = nullptr;  // clear kinds: the bytes the extract-sums read,
    size_t text_n = 0;              // and how many (a find: n; a scan: n windows of m bytes)
    Sink sink = ToHandles{nullptr, nullptr};

    bool clear() const { return kind == MATCH_NEEDLE_CLEAR || kind == MATCH_NEEDLE_WINDOWS; }
};

// ------------------------------------------------------------ plan cache
// The circuit of a match is data-oblivious: it depends on (pattern, grammar,
// engine, lowering, multi-value, length, start range, batch size) and on the
// content's *shape* -- which blocks are trivial and their values, and which
// positions share a ciphertext (the multi-value merge compares inputs) -- never on
// the ciphertexts themselves.  A cached plan is a template plan (Plan::n_refs):
// its content inputs are references that each call binds to the call's arena
// slots through a content map, so a fresh ciphertext of the same shape replays
// the plan (the reference re-plans every call, engine.rs:8-42).  A cached plan
// keeps its intermediate slots and a device copy of its gate batches; a repeat
// call skips parse -> record -> lower -> compile and the descriptor uploads, and
// only binds the content and enqueues the levels.  The cache is bounded by entries
// (LRU, default 8, FR_PLAN_CACHE) and by the intermediate slots it holds (default
// 2^18 = 4.3 GB at k = 1, FR_PLAN_CACHE_SLOTS); eviction runs before the new plan
// allocates, and a plan larger than the slot budget runs uncached.

// The key is a fixed number of '|'-terminated numeric fields followed by the pattern, so a
// pattern's own text (which may contain '|' and digits) cannot make two keys collide.
// needle_m > 0: a private search (fr_find*) for a needle of that many characters, the pattern
// empty -- the plan does not depend on the needle's ciphertext, so the length stands for it.
// clear: that search over clear content (fr_find_clear*), whose plan does not depend on the
// content's bytes either; the field keeps it apart from fr_find's plan for the same (m, n).  A
// scan (fr_scan_clear*) is the field's third value with n its padded class count, so its plan is
// never fr_find_clear's for the same numbers.  form: the needle's (nibbles 0, byte tables 1), so a
// byte needle of (m, n) never replays a nibble needle's plan.
std::string match_key(const fr_ctx* ctx, const MatchRequest& rq, int lane) {
    const size_t needle_m = rq.needle ? rq.needle->dev.m : 0, form = rq.needle ? (size_t)rq.needle->dev.form : 0;
    const size_t clear = rq.kind == MATCH_NEEDLE_CLEAR ? 1 : rq.kind == MATCH_NEEDLE_WINDOWS ? 2 : 0;
    std::string k;
    for (size_t v : {(size_t)ctx->grammar, (size_t)ctx->engine, (size_t)ctx->lowering, (size_t)ctx->multi_value, rq.n,
                     rq.M, rq.lo, rq.hi, rq.parts, (size_t)lane, (size_t)rq.starts, needle_m, clear, form})
        k += std::to_string(v) + "|";
    k += rq.pattern;
    return k;
}
// Canonical shape of the content: per position and block, the trivial value
// (-1 - v), the index of the block's ciphertext in order of first appearance (>= 0:
// equal indices = the same arena slot), or markers for an absent position / a
// boolean handle.  Two contents with equal signatures lower, schedule and merge
// identically.  cmap (if given) receives the content map: block r -> slot (-1: none).
std::vector<int32_t> content_signature(fr_ctx* ctx, const fr_ct* content, size_t n, std::vector<int>* cmap) {
    constexpr int32_t ABSENT = INT32_MIN, BOOL = INT32_MIN + 1;
    std::vector<int32_t> sig;
    sig.reserve(4 * n);
    if (cmap) cmap->assign(4 * n, -1);
    if (++ctx->gen == 0) {  // generation wrapped: forget every stamp
        std::fill(ctx->sig_gen.begin(), ctx->sig_gen.end(), 0u);
        ctx->gen = 1;
    }
    int32_t next_id = 0;
    for (size_t q = 0; q < n; ++q) {
        if (content[q] == 0xFFFFFFFFu) {
            sig.insert(sig.end(), 4, ABSENT);
            continue;
        }
        const HandleRec& h = ctx->get(content[q]);
        for (int b = 0; b < 4; ++b) {
            const int s = h.b[b].slot;
            if (h.is_bool) {
                sig.push_back(BOOL);
            } else if (s < 0) {
                sig.push_back(-1 - (int32_t)h.b[b].triv);
            } else {
                if ((size_t)s >= ctx->sig_id.size()) {
                    ctx->sig_id.resize((size_t)s + 1024);
                    ctx->sig_gen.resize((size_t)s + 1024, 0u);
                }
                if (ctx->sig_gen[s] != ctx->gen) {
                    ctx->sig_gen[s] = ctx->gen;
                    ctx->sig_id[s] = next_id++;
                }
                sig.push_back(ctx->sig_id[s]);
            }
            if (cmap) (*cmap)[4 * q + b] = s;
        }
    }
    return sig;
}

// entry i goes: its plan waits for every lane, then gives its slots and its batch back (Plan)
void drop_cached(fr_plan_cache& pc, size_t i) {
    pc.slots_held -= std::min(pc.slots_held, pc.entries[i]->plan.slot.size());
    pc.entries.erase(pc.entries.begin() + (long)i);
}
// drop least-recently-used plans until `entries` and `slots` more fit
void evict_for(fr_ctx* ctx, size_t entries, size_t slots) {
    fr_plan_cache& pc = ctx->plans;
    while (!pc.entries.empty() &&
           (pc.entries.size() + entries > pc.capacity || pc.slots_held + slots > pc.slot_cap)) {
        size_t v = 0;
        for (size_t i = 1; i < pc.entries.size(); ++i)
            if (pc.entries[i]->last_use < pc.entries[v]->last_use) v = i;
        drop_cached(pc, v);
    }
}

// the content handles a program reads, for each of M matches over n positions
// (content[m * n + q]): every one present and a radix character
void check_content(fr_ctx* ctx, const Program& prog, const fr_ct* content, size_t n, size_t M) {
    for (auto& g : prog.gates)
        for (auto& in : g.ins)
            if (in.src < 0) {
                const size_t q = (size_t)((-in.src - 1) / 4);
                for (size_t m = 0; m < M; ++m) {
                    const fr_ct c = q < n ? content[m * n + q] : 0xFFFFFFFFu;
                    if (c == 0xFFFFFFFFu) throw Error(FR_ERR_INVALID, "content position not provided");
                    if (ctx->get(c).is_bool) throw Error(FR_ERR_INVALID, "content handle is not a radix character");
                }
            }
}

// the front end's input for a context's settings
MatchSpec match_spec(const fr_ctx* ctx, const char* pattern, size_t n, size_t lo, size_t hi, size_t parts = 1) {
    return MatchSpec{pattern, n, lo, hi, ctx->engine, ctx->grammar, ctx->lowering, (int)parts};
}

// the counters of a recording and of its plan, into zeroed stats
void fill_stats(fr_match_stats& s, const Recorded& rec, const Plan& P) {
    s.ct_ops = rec.ct_ops;
    s.cache_hits = rec.cache_hits;
    s.n_branches = rec.n_branches;
    add_plan_stats(P, &s);
}

// the bytes of a scan's reply over n_starts starts
size_t scan_reply_size(const Params& p, size_t n_starts, bool compact) {
    size_t need = 0;
    for (size_t j0 = 0; j0 < n_starts; j0 += (size_t)p.N)
        need += compact ? packed_compact_size(p, std::min((size_t)p.N, n_starts - j0)) : packed_result_size(p);
    return need;
}
// refused before anything is planned or launched
void check_needle(fr_ctx* ctx, Device& dev, const fr_needle* needle) {
    if (ctx->p.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "private search: FFT ring only");
    if (needle->k != ctx->p.k || needle->N != ctx->p.N)
        throw Error(FR_ERR_INVALID, "needle: k, N do not match the context params");
    if (needle->dev.dev != &dev || !needle->dev.words) throw Error(FR_ERR_INVALID, "needle: uploaded to another context");
}
// ... and so is a byte-table needle over encrypted content: those searches rotate the tables
void check_needle_kind(const MatchRequest& rq) {
    if (rq.kind == MATCH_NEEDLE && rq.needle->dev.form == NEEDLE_BYTES)
        throw Error(FR_ERR_INVALID, "needle: a byte-table needle searches clear content only");
}

// Every legality rule of a request, before anything is planned or launched.
void validate(const MatchRequest& rq) {
    if (rq.M == 0) throw Error(FR_ERR_INVALID, "no matches");
    if ((rq.kind != MATCH_PATTERN) != (rq.needle != nullptr))
        throw Error(FR_ERR_INVALID, "a needle kind has a needle, a pattern none");
    if (rq.clear() && (rq.M != 1 || rq.content)) throw Error(FR_ERR_INVALID, "clear content: one needle, no handles");
    if (!std::holds_alternative<ToHandles>(rq.sink) && (!rq.starts || rq.M != 1))
        throw Error(FR_ERR_INVALID, "a packed reply holds the starts of one match");
    if (std::holds_alternative<ToScanBlobs>(rq.sink) && rq.kind != MATCH_NEEDLE_WINDOWS)
        throw Error(FR_ERR_INVALID, "chunked blobs are a scan's reply");
}

// ------------------------------------------------------------ stage 1: the plan
// The one place that maps a request to its compile function: the lowered program of one match
// and the recording's counters (a needle search records nothing).
struct Compiled {
    Program prog;
    Recorded rec;
};
Compiled program_for(const fr_ctx* ctx, const MatchRequest& rq) {
    if (rq.kind != MATCH_PATTERN)
        return {needle_program(rq.kind, rq.n, rq.needle->dev.m, rq.lo, rq.hi, rq.starts,
                               rq.needle->dev.form == NEEDLE_BYTES),
                Recorded{}};
    if (rq.starts) {
        CompiledStarts cs = compile_match_starts(match_spec(ctx, rq.pattern, rq.n, rq.lo, rq.hi));
        return {std::move(cs.prog), cs.rec};
    }
    CompiledMatch cm = compile_match(match_spec(ctx, rq.pattern, rq.n, rq.lo, rq.hi, rq.parts));
    return {std::move(cm.prog), cm.rec};
}

// M copies of one match's gates, so every level of the M matches shares its launches: gate g of
// match m is m * G + g, content block cb of match m is 4 n m + cb
std::vector<PGate> fold_gates(const std::vector<PGate>& one, size_t n, size_t M) {
    const size_t G = one.size();
    std::vector<PGate> gates;
    gates.reserve(G * M);
    for (size_t m = 0; m < M; ++m)
        for (const PGate& g0 : one) {
            PGate g = g0;
            for (auto& in : g.ins) in.src = in.src >= 0 ? in.src + (int)(m * G) : in.src - (int)(4 * n * m);
            gates.push_back(std::move(g));
        }
    return gates;
}

// What a request runs: c holds the plan, one match's outputs and gate count and the recording's
// counters.  It is the cache's entry (a hit, or this call's plan once kept) or, for a plan that
// runs uncached, the call's own.
struct PlanView {
    CachedMatch* c = nullptr;
    std::unique_ptr<CachedMatch> own;
    bool hit = false;
    int lane = 0;           // the lane a cached plan runs on
    std::vector<int> cmap;  // the call's content map, for a cached plan's references
};
PlanView acquire_plan(fr_ctx* ctx, Device& dev, const MatchRequest& rq) {
    fr_plan_cache& pc = ctx->plans;
    PlanView v;
    const size_t n_handles = rq.clear() ? 0 : rq.n * rq.M;
    // lanes (fr_set_lanes): an asynchronous match of a cacheable plan runs on the next lane,
    // with a plan of its own (its intermediate slots), so consecutive matches overlap
    v.lane =
        (ctx->async_match && dev.match_lanes() > 0 && pc.capacity) ? 1 + (int)(ctx->next_lane++ % dev.match_lanes()) : 0;
    std::string key;
    std::vector<int32_t> sig;
    if (pc.capacity) {
        key = match_key(ctx, rq, v.lane);
        sig = content_signature(ctx, rq.content, n_handles, &v.cmap);
        for (auto& e : pc.entries)
            if (e->parts == rq.parts && e->lane == v.lane && e->key == key && e->sig == sig) v.c = e.get();
    }
    if (v.c) {
        v.hit = true;
        ++pc.hits;
        v.c->last_use = ++pc.clock;
        return v;
    }
    ++pc.misses;  // (counted even if the request then fails to compile)
    Compiled cp = program_for(ctx, rq);
    if (!rq.clear()) check_content(ctx, cp.prog, rq.content, rq.n, rq.M);
    const size_t G = cp.prog.gates.size();
    const std::vector<PGate> gates = fold_gates(cp.prog.gates, rq.n, rq.M);
    const bool keep = pc.capacity && G && G * rq.M <= pc.slot_cap;
    if (keep) evict_for(ctx, 1, G * rq.M);  // before the new plan allocates its slots
    auto e = std::make_unique<CachedMatch>();
    e->plan = compile_plan(ctx, gates, std::vector<fr_ct>(rq.content, rq.content + n_handles), keep, rq.text_n);
    e->key = std::move(key);
    e->parts = rq.parts;
    e->lane = v.lane;
    e->sig = std::move(sig);
    e->n_gates = G;
    e->outs = std::move(cp.prog.outs);
    e->rec = cp.rec;
    v.c = e.get();
    if (!keep) {
        v.own = std::move(e);
        return v;
    }
    // keep the plan: its slots stay allocated, its batches go to the device once; the entry is
    // complete before the cache sees it
    e->last_use = ++pc.clock;
    e->plan.d_gates = dev.upload_gates(e->plan.gates.data(), e->plan.gates.size(), e->plan.n_refs);
    if (!e->plan.sums.empty()) e->plan.d_sums = dev.upload_sums(e->plan.sums.data(), e->plan.sums.size());
    pc.entries.push_back(std::move(e));
    pc.slots_held += v.c->plan.slot.size();
    return v;
}

// ------------------------------------------------------------ stage 2: the launch
// This match's lane, content map, selector table and text: bound in that order around its
// launches and its emit, and let go on every exit, exceptions included.
struct Bound {
    Device& d;
    bool lane = false, selectors = false, text = false;
    // a cached plan runs on its lane, its content references bound to the call's slots
    void plan(const PlanView& v) {
        if (v.own) return;
        if (v.lane > 0) d.enter_lane(v.lane), lane = true;
        d.bind_content(v.cmap.data(), v.cmap.size());
    }
    // the needle's table and the clear content, for this match's launches on this lane only
    void search(const MatchRequest& rq) {
        selectors = rq.needle != nullptr, text = rq.clear();
        if (selectors) d.bind_selectors(rq.needle->dev.words.get(), rq.needle->dev.tables(), rq.needle->dev.form);
        // the call's bytes, copied now and in stream order on this lane: the caller's buffer may go
        if (text) d.bind_text(rq.text, rq.text_n);
    }
    ~Bound() {
        if (selectors) d.bind_selectors(nullptr, 0);
        try {
            if (text) d.bind_text(nullptr, 0);
        } catch (...) {
        }
        if (lane) d.leave_lane();
    }
};
// enqueues the plan, bound to its match; returns when the call's host part ended (the plan bound)
double launch(Bound& bound, const PlanView& v, const MatchRequest& rq) {
    bound.plan(v);
    const double t1 = now_ms();
    bound.search(rq);
    launch_plan(bound.d, v.c->plan);
    return t1;
}

// ------------------------------------------------------------ stage 3: the reply
// All three run inside the launch's scope: a pack follows the plan's launches on this lane's
// stream, uses this lane's scratch and waits for this stream only.

// handles: outs[m * P + j] for the P outputs of each of the M matches
void emit(fr_ctx* ctx, PlanView& v, const MatchRequest& rq, const ToHandles& to) {
    const std::vector<ProgOut>& po = v.c->outs;
    const size_t nO = po.size();
    if (v.hit && !rq.starts && (nO < 1 || nO > rq.parts))  // the caller's out buffer holds M * parts handles
        throw Error(FR_ERR_INVALID, "cached plan has more outputs than the caller's parts");
    // an uncached plan's one output takes its gate's slot; parts get copies (two parts may read one gate)
    const bool take = v.own && nO == 1;
    size_t made = 0;  // handles written so far, released if a later one fails: the caller gets a code only
    try {
        for (size_t m = 0; m < rq.M; ++m)
            for (size_t j = 0; j < nO; ++j, ++made) {
                ProgOut o = po[j];
                if (o.gate >= 0) o.gate += (int)(m * v.c->n_gates);
                to.outs[m * nO + j] = make_output(ctx, o, v.c->plan.slot, take);
            }
    } catch (...) {
        while (made) ctx->release(to.outs[--made]);
        throw;
    }
    if (to.n_parts) *to.n_parts = nO;
}

// Each output o.cst + o.w * gate as a pack row over the plan's own gate slot (a constant start:
// no input), so no handle, no arena slot and no k_linear launch stands between the plan and the
// pack.  One per start of the request, or the plan is not this request's.
std::vector<DevGate> output_rows(const PlanView& v, const MatchRequest& rq) {
    const std::vector<ProgOut>& po = v.c->outs;
    if (po.size() != rq.hi - rq.lo) throw Error(FR_ERR_INVALID, "cached plan's outputs are not the call's starts");
    std::vector<DevGate> rows(po.size());
    for (size_t j = 0; j < po.size(); ++j)
        rows[j] = affine_gate(po[j].gate >= 0 ? v.c->plan.slot[po[j].gate] : -1, po[j].w, po[j].cst);
    return rows;
}
void emit(fr_ctx* ctx, PlanView& v, const MatchRequest& rq, const ToBlob& to) {
    const std::vector<DevGate> rows = output_rows(v, rq);
    pack_to_blob(ctx, rows.data(), rows.size(), nullptr, rows.size(), to.compact, to.buf);
}

// One chunk of a scan's starts, on the host alone: `classes` are the classes that occur among
// cls[0, nc) in order of first occurrence (the chunk's rows) and map[j] is the row of start j
// (-1: the constant 0).  The numbering is the chunk's own.  row_of is scratch over the n_classes
// classes, all -1 before and after.
void chunk_classes(const int32_t* cls, size_t nc, size_t n_classes, std::vector<int32_t>& row_of,
                   std::vector<int32_t>& classes, std::vector<int32_t>& map) {
    classes.clear();
    map.assign(nc, -1);
    for (size_t j = 0; j < nc; ++j) {
        const int32_t d = cls[j];
        if (d < 0) continue;
        if ((size_t)d >= n_classes) throw Error(FR_ERR_INVALID, "scan: a class past the plan's outputs");
        if (row_of[(size_t)d] < 0) {
            row_of[(size_t)d] = (int32_t)classes.size();
            classes.push_back(d);
        }
        map[j] = row_of[(size_t)d];
    }
    for (int32_t d : classes) row_of[(size_t)d] = -1;
}
// a scan: the plan's outputs are window classes; one mapped pack per chunk of N starts, the
// blobs back to back (no start at all: cls may be null, and no chunk is written)
void emit(fr_ctx* ctx, PlanView& v, const MatchRequest& rq, const ToScanBlobs& to) {
    const std::vector<DevGate> outs = output_rows(v, rq);
    const size_t N = (size_t)ctx->p.N;
    std::vector<int32_t> row_of(outs.size(), -1), classes, map;
    std::vector<DevGate> rows;
    uint8_t* at = to.buf;
    for (size_t j0 = 0; j0 < to.n_starts; j0 += N) {
        const size_t nc = std::min(N, to.n_starts - j0);
        chunk_classes(to.cls + j0, nc, outs.size(), row_of, classes, map);
        rows.clear();
        for (int32_t d : classes) rows.push_back(outs[(size_t)d]);
        at += pack_to_blob(ctx, rows.data(), rows.size(), map.data(), nc, to.compact, at);
    }
}

// after: the device's timers once a blocking call has synchronised, which resolved this match's;
// null for an asynchronous call, which returns before its kernels ran: its kernel timers are
// left 0 (read them with fr_device_timers after a synchronising call instead)
void match_stats(fr_match_stats* st, const DeviceTimers& before, const DeviceTimers* after, double t0, double t1,
                 double t2, const PlanView& v) {
    std::memset(st, 0, sizeof *st);
    fill_stats(*st, v.c->rec, v.c->plan);
    st->host_ms = t1 - t0;
    st->device_ms = t2 - t1;
    st->plan_cached = v.hit ? 1 : 0;
    if (!after) return;
    st->br_kernel_ms = after->br_ms - before.br_ms;
    st->ks_kernel_ms = after->ks_ms - before.ks_ms;
    st->br_launches = after->br_launches - before.br_launches;
    st->br_gates = after->br_gates - before.br_gates;
}

// One match request through its stages: the plan, the launch, the reply.
void run_match(fr_ctx* ctx, const MatchRequest& rq, fr_match_stats* st) {
    const double t0 = now_ms();
    Device& dev = ctx->keyed_device();
    validate(rq);
    if (rq.needle) check_needle(ctx, dev, rq.needle), check_needle_kind(rq);
    const DeviceTimers before = dev.timers();
    PlanView v = acquire_plan(ctx, dev, rq);
    Bound bound{dev};
    const double t1 = launch(bound, v, rq);
    std::visit([&](const auto& to) { emit(ctx, v, rq, to); }, rq.sink);
    if (v.own) v.own->plan.slot.reset();  // later users of these slots are ordered after the launches (one stream)
    if (!ctx->async_match) dev.sync();
    if (st) match_stats(st, before, ctx->async_match ? nullptr : &dev.timers(), t0, t1, now_ms(), v);
}

// a pattern's request over n content handles and the starts of [lo, hi)
MatchRequest pattern_request(const fr_ct* content, size_t n, const char* pattern, size_t lo, size_t hi, Sink sink) {
    MatchRequest rq;
    rq.pattern = pattern;
    rq.content = content;
    rq.n = n, rq.lo = lo, rq.hi = hi;
    rq.sink = sink;
    return rq;
}
// a needle's request of one kind over n positions (windows: n classes, the whole range); the
// entry adds what the kind reads, content handles or text
MatchRequest needle_request(MatchKind kind, const fr_needle* needle, size_t n, size_t lo, size_t hi, Sink sink) {
    MatchRequest rq;
    rq.kind = kind;
    rq.needle = needle;
    rq.n = n, rq.lo = lo, rq.hi = hi;
    rq.sink = sink;
    return rq;
}

// A scan's host part: the classes of the starts of [lo, hi), the padded class count and the text
// the plan reads (pad_window_text).  The counts are left in the context for fr_scan_classes.
WindowClasses scan_windows(fr_ctx* ctx, const uint8_t* content, size_t n_chars, size_t m, size_t lo, size_t hi,
                           size_t* Dpad) {
    if (n_chars > (size_t)1 << 24) throw Error(FR_ERR_INVALID, "scan: content longer than 2^24");
    WindowClasses wc = window_classes(content, n_chars, m, lo, hi);
    *Dpad = scan_padded(wc.first.size());
    if (*Dpad * m > (size_t)1 << 24) throw Error(FR_ERR_INVALID, "scan: more than 2^24 window bytes");
    pad_window_text(wc, m);
    ctx->scan_classes = wc.first.size();
    ctx->scan_padded = *Dpad;
    return wc;
}

}  // namespace

extern "C" {

int fr_has_match(fr_ctx* ctx, const fr_ct* content, size_t n, const char* pattern, fr_ct* out, fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && out && pattern && (content || !n));
        run_match(ctx, pattern_request(content, n, pattern, 0, n, ToHandles{out, nullptr}), st);
    })
}

int fr_set_plan_cache(fr_ctx* ctx, size_t capacity) {
    FR_TRY({
        NEED(ctx);
        ctx->plans.capacity = capacity;
        evict_for(ctx, 0, 0);  // drop the least recently used beyond the new capacity
    })
}

int fr_set_lanes(fr_ctx* ctx, int32_t n) {
    FR_TRY({
        NEED(ctx && n >= 1 && n <= 8);
        Device& dev = ctx->device();
        if (n == 1 ? dev.match_lanes() == 0 : dev.match_lanes() == n) return FR_OK;
        // the lanes' plan copies go with the lanes (their slots are held by the cache)
        fr_plan_cache& pc = ctx->plans;
        for (size_t i = pc.entries.size(); i-- > 0;)
            if (pc.entries[i]->lane != 0) drop_cached(pc, i);
        dev.set_lanes(n);
        ctx->next_lane = 0;
    })
}

int fr_set_async(fr_ctx* ctx, int32_t on) {
    FR_TRY({
        NEED(ctx);
        ctx->async_match = on != 0;
    })
}

int fr_set_plan_cache_slots(fr_ctx* ctx, size_t max_slots) {
    FR_TRY({
        NEED(ctx);
        ctx->plans.slot_cap = max_slots;
        evict_for(ctx, 0, 0);
    })
}

int fr_plan_cache_stats(fr_ctx* ctx, uint64_t* entries, uint64_t* slots, uint64_t* hits, uint64_t* misses) {
    FR_TRY({
        NEED(ctx);
        const fr_plan_cache& pc = ctx->plans;
        if (entries) *entries = pc.entries.size();
        if (slots) *slots = pc.slots_held;
        if (hits) *hits = pc.hits;
        if (misses) *misses = pc.misses;
    })
}

int fr_has_match_batch(fr_ctx* ctx, const fr_ct* content, size_t n_chars, size_t n_matches, const char* pattern,
                       fr_ct* out, fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && out && pattern && n_matches && (content || !n_chars));
        MatchRequest rq = pattern_request(content, n_chars, pattern, 0, n_chars, ToHandles{out, nullptr});
        rq.M = n_matches;
        run_match(ctx, rq, st);
    })
}

int fr_has_match_range(fr_ctx* ctx, const fr_ct* content, size_t n, const char* pattern, size_t lo, size_t hi,
                       fr_ct* out, fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && out && pattern && (content || !n) && lo <= hi);
        run_match(ctx, pattern_request(content, n, pattern, lo, hi, ToHandles{out, nullptr}), st);
    })
}

int fr_match_starts(fr_ctx* ctx, const fr_ct* content, size_t n, const char* pattern, size_t lo, size_t hi, fr_ct* out,
                    fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && pattern && (content || !n) && lo <= hi && (out || lo == hi));
        // (the key's `starts` field keeps these plans apart from has_match's of the same range)
        MatchRequest rq = pattern_request(content, n, pattern, lo, hi, ToHandles{out, nullptr});
        rq.starts = true;
        run_match(ctx, rq, st);
    })
}

int fr_match_starts_packed(fr_ctx* ctx, const fr_ct* content, size_t n, const char* pattern, size_t lo, size_t hi,
                           int32_t compact, uint8_t* buf, size_t cap, size_t* written, fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && pattern && written && (content || !n) && lo < hi && hi - lo <= (size_t)ctx->p.N);
        NEED(compact == 0 || compact == 1);
        ctx->keyed_device();  // a host-only or keyless context refuses as fr_match_starts does
        ctx->need_packing_key();  // ... and nothing is launched without a packing key
        const size_t need = compact ? packed_compact_size(ctx->p, hi - lo) : packed_result_size(ctx->p);
        if (answer_size(written, need, buf, cap)) return FR_OK;
        // the plans are fr_match_starts' own (same key): one compiled by either call serves the other
        MatchRequest rq = pattern_request(content, n, pattern, lo, hi, ToBlob{compact != 0, buf});
        rq.starts = true;
        run_match(ctx, rq, st);
    })
}

int fr_find(fr_ctx* ctx, const fr_ct* content, size_t n_chars, const fr_needle* needle, size_t start_lo,
            size_t start_hi, fr_ct* out, fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && needle && out && (content || !n_chars) && start_lo <= start_hi);
        // no start past the content fits: the range is cut there (one plan for every such range)
        const size_t hi = std::min(start_hi, n_chars), lo = std::min(start_lo, hi);
        MatchRequest rq = needle_request(MATCH_NEEDLE, needle, n_chars, lo, hi, ToHandles{out, nullptr});
        rq.content = content;
        run_match(ctx, rq, st);
    })
}

int fr_find_starts(fr_ctx* ctx, const fr_ct* content, size_t n_chars, const fr_needle* needle, size_t start_lo,
                   size_t start_hi, fr_ct* out, fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && needle && (content || !n_chars) && start_lo <= start_hi && (out || start_lo == start_hi));
        NEED(start_hi - start_lo <= ((size_t)1 << 24));
        MatchRequest rq = needle_request(MATCH_NEEDLE, needle, n_chars, start_lo, start_hi, ToHandles{out, nullptr});
        rq.starts = true;
        rq.content = content;
        run_match(ctx, rq, st);
    })
}

int fr_find_clear(fr_ctx* ctx, const uint8_t* content, size_t n_chars, const fr_needle* needle, size_t start_lo,
                  size_t start_hi, fr_ct* out, fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && needle && out && (content || !n_chars) && start_lo <= start_hi);
        // (the range is cut at the content's end, as fr_find cuts it)
        const size_t hi = std::min(start_hi, n_chars), lo = std::min(start_lo, hi);
        MatchRequest rq = needle_request(MATCH_NEEDLE_CLEAR, needle, n_chars, lo, hi, ToHandles{out, nullptr});
        rq.text = content, rq.text_n = n_chars;
        run_match(ctx, rq, st);
    })
}

int fr_find_clear_starts(fr_ctx* ctx, const uint8_t* content, size_t n_chars, const fr_needle* needle, size_t start_lo,
                         size_t start_hi, fr_ct* out, fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && needle && (content || !n_chars) && start_lo <= start_hi && (out || start_lo == start_hi));
        NEED(start_hi - start_lo <= ((size_t)1 << 24));
        MatchRequest rq =
            needle_request(MATCH_NEEDLE_CLEAR, needle, n_chars, start_lo, start_hi, ToHandles{out, nullptr});
        rq.starts = true;
        rq.text = content, rq.text_n = n_chars;
        run_match(ctx, rq, st);
    })
}

int fr_scan_clear(fr_ctx* ctx, const uint8_t* content, size_t n_chars, const fr_needle* needle, size_t start_lo,
                  size_t start_hi, fr_ct* out, fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && needle && out && (content || !n_chars) && start_lo <= start_hi);
        check_needle(ctx, ctx->keyed_device(), needle);  // before the text is classed
        const size_t hi = std::min(start_hi, n_chars), lo = std::min(start_lo, hi);
        size_t Dpad = 0;
        const double t0 = now_ms();
        const WindowClasses wc = scan_windows(ctx, content, n_chars, needle->dev.m, lo, hi, &Dpad);
        const double classing_ms = now_ms() - t0;
        MatchRequest rq = needle_request(MATCH_NEEDLE_WINDOWS, needle, Dpad, 0, Dpad, ToHandles{out, nullptr});
        rq.text = wc.text.data(), rq.text_n = wc.text.size();
        run_match(ctx, rq, st);
        if (st) st->host_ms += classing_ms;  // the classing is the scan's host work too
    })
}

int fr_scan_clear_starts(fr_ctx* ctx, const uint8_t* content, size_t n_chars, const fr_needle* needle, size_t start_lo,
                         size_t start_hi, int32_t compact, uint8_t* buf, size_t cap, size_t* written,
                         fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && needle && written && (content || !n_chars) && start_lo <= start_hi);
        NEED(compact == 0 || compact == 1);
        NEED(start_hi - start_lo <= ((size_t)1 << 24));
        check_needle(ctx, ctx->keyed_device(), needle);  // a host-only or keyless context refuses as fr_find_clear does
        ctx->need_packing_key();                         // ... and nothing is launched without a packing key
        const size_t n_starts = start_hi - start_lo;
        if (answer_size(written, scan_reply_size(ctx->p, n_starts, compact != 0), buf, cap)) return FR_OK;
        size_t Dpad = 0;
        const double t0 = now_ms();
        WindowClasses wc = scan_windows(ctx, content, n_chars, needle->dev.m, start_lo, start_hi, &Dpad);
        wc.cls.resize(n_starts, -1);  // a start past the content: the constant 0
        const double classing_ms = now_ms() - t0;
        MatchRequest rq = needle_request(MATCH_NEEDLE_WINDOWS, needle, Dpad, 0, Dpad,
                                         ToScanBlobs{compact != 0, buf, wc.cls.data(), n_starts});
        rq.starts = true;
        rq.text = wc.text.data(), rq.text_n = wc.text.size();
        run_match(ctx, rq, st);
        if (st) st->host_ms += classing_ms;
    })
}

int fr_scan_classes(fr_ctx* ctx, uint64_t* classes, uint64_t* padded) {
    FR_TRY({
        NEED(ctx);
        if (classes) *classes = ctx->scan_classes;
        if (padded) *padded = ctx->scan_padded;
    })
}

int fr_has_match_parts(fr_ctx* ctx, const fr_ct* content, size_t n, const char* pattern, size_t lo, size_t hi,
                       size_t max_parts, fr_ct* out, size_t* n_parts, fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && out && n_parts && pattern && (content || !n) && lo <= hi);
        NEED(max_parts >= 1 && max_parts <= (size_t)MAX_FANIN);
        MatchRequest rq = pattern_request(content, n, pattern, lo, hi, ToHandles{out, n_parts});
        rq.parts = max_parts;
        run_match(ctx, rq, st);
    })
}

}  // extern "C"

// the schedule of a lowered program over n_chars encrypted characters (each position an
// encrypted radix character), and its outputs as (gate, w, cst) triples
// (in_slot of a job that reads an extract-sum is that sum's gate index, as for any gate)
static void schedule_program(const Program& prog, size_t n_chars, int32_t multi_value, fr_job* jobs, size_t jobs_cap,
                             size_t* n_jobs, uint32_t* level_off, size_t level_cap, size_t* n_levels, int32_t* outs3,
                             size_t* n_parts) {
    Schedule S = build_schedule(prog.gates, n_chars, multi_value != 0, [](int cb, int& key, int&) {
        key = cb;
        return true;
    }, n_chars);
    *n_jobs = S.jobs.size();
    *n_levels = S.level_off.size() - 1;
    *n_parts = prog.outs.size();
    for (size_t j = 0; j < prog.outs.size(); ++j) {
        outs3[3 * j] = prog.outs[j].gate;
        outs3[3 * j + 1] = prog.outs[j].w;
        outs3[3 * j + 2] = prog.outs[j].cst;
    }
    if (jobs) {
        NEED(jobs_cap >= S.jobs.size());
        static_assert(sizeof(fr_job) == sizeof(DevGate), "fr_job mirrors DevGate");
        // (an empty schedule's vector has no storage: memcpy's source must not be null,
        // UBSan finding of tests/test_fuzz_inputs.py)
        if (!S.jobs.empty()) std::memcpy(jobs, S.jobs.data(), sizeof(DevGate) * S.jobs.size());
    }
    if (level_off) {
        NEED(level_cap >= S.level_off.size());
        for (size_t l = 0; l < S.level_off.size(); ++l) level_off[l] = (uint32_t)S.level_off[l];
    }
}

// ------------------------------------------------------------ level-sharded matches
// One match split across ranks (the reference folds ct_or over the
// start offsets of engine.rs:15-35, and anchored patterns have a single start,
// engine.rs:51-57): every rank compiles the same plan over its own copy of the
// content, runs a contiguous slice of every level's rotation jobs, and all-gathers
// the level's output LWEs device to device (fr_shard_export / fr_shard_import into
// the caller's device buffers, e.g. RCCL all_gather); every rank then holds the
// level's outputs and goes on to the next.  The plan keeps its slots and a device
// copy of its batches, so repeat runs only enqueue.
struct fr_shard {
    Plan plan;
    ProgOut out;
    std::vector<std::vector<int>> out_slots;     // per level: output slots in job order
    std::vector<std::vector<uint32_t>> out_off;  // per level: first output of each job (+ total)
    fr_match_stats stats{};
};

static const std::vector<int>& shard_level_range(const fr_shard* sh, uint32_t level, uint32_t b, uint32_t e,
                                                 uint32_t& first, uint32_t& count) {
    if (level >= sh->out_off.size()) throw Error(FR_ERR_INVALID, "shard: level out of range");
    const auto& off = sh->out_off[level];
    if (b > e || e + 1 > off.size()) throw Error(FR_ERR_INVALID, "shard: job range out of range");
    first = off[b];
    count = off[e] - off[b];
    return sh->out_slots[level];
}

extern "C" {

int fr_shard_plan(fr_ctx* ctx, const fr_ct* content, size_t n, const char* pattern, size_t lo, size_t hi,
                  fr_shard** out, fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && out && pattern && (content || !n) && lo <= hi);
        Device& dev = ctx->keyed_device();
        const double t0 = now_ms();
        const CompiledMatch cm = compile_match(match_spec(ctx, pattern, n, lo, hi));
        const Recorded& rec = cm.rec;
        const Program& prog = cm.prog;
        check_content(ctx, prog, content, n, 1);
        auto sh = std::make_unique<fr_shard>();
        sh->plan = compile_plan(ctx, prog.gates, std::vector<fr_ct>(content, content + n));
        Plan& P = sh->plan;
        P.d_gates = dev.upload_gates(P.gates.data(), P.gates.size());
        sh->out = prog.outs[0];
        for (size_t l = 0; l + 1 < P.level_off.size(); ++l) {
            std::vector<int> slots;
            std::vector<uint32_t> off{0};
            for (size_t j = P.level_off[l]; j < P.level_off[l + 1]; ++j) {
                for (int f = 0; f < P.gates[j].n_out; ++f) slots.push_back(P.gates[j].out_slot[f]);
                off.push_back((uint32_t)slots.size());
            }
            sh->out_slots.push_back(std::move(slots));
            sh->out_off.push_back(std::move(off));
        }
        fill_stats(sh->stats, rec, P);
        sh->stats.host_ms = now_ms() - t0;
        if (st) *st = sh->stats;
        *out = sh.release();
    })
}
int fr_shard_levels(const fr_shard* sh, uint32_t* levels) {
    FR_TRY({
        NEED(sh && levels);
        *levels = (uint32_t)sh->out_off.size();
    })
}
int fr_shard_jobs(const fr_shard* sh, uint32_t level, uint32_t* jobs) {
    FR_TRY({
        NEED(sh && jobs && level < sh->out_off.size());
        *jobs = (uint32_t)sh->out_off[level].size() - 1;
    })
}
int fr_shard_outputs(const fr_shard* sh, uint32_t level, uint32_t begin, uint32_t end, uint32_t* n_lwe) {
    FR_TRY({
        NEED(sh && n_lwe);
        uint32_t first, count;
        shard_level_range(sh, level, begin, end, first, count);
        *n_lwe = count;
    })
}
int fr_shard_run(fr_ctx* ctx, fr_shard* sh, uint32_t level, uint32_t begin, uint32_t end) {
    FR_TRY({
        NEED(ctx && sh);
        uint32_t first, count;
        shard_level_range(sh, level, begin, end, first, count);
        const Plan& P = sh->plan;
        const size_t a = P.level_off[level] + begin;
        ctx->device().run_level_resident(P.d_gates.get() + a, P.gates.data() + a, end - begin);
    })
}
int fr_shard_export(fr_ctx* ctx, fr_shard* sh, uint32_t level, uint32_t begin, uint32_t end, uint64_t* dev_dst) {
    FR_TRY({
        NEED(ctx && sh);
        uint32_t first, count;
        const std::vector<int>& slots = shard_level_range(sh, level, begin, end, first, count);
        NEED(dev_dst || !count);
        ctx->device().slots_to_device(slots.data() + first, count, dev_dst);
    })
}
int fr_shard_import(fr_ctx* ctx, fr_shard* sh, uint32_t level, uint32_t begin, uint32_t end, const uint64_t* dev_src) {
    FR_TRY({
        NEED(ctx && sh);
        uint32_t first, count;
        const std::vector<int>& slots = shard_level_range(sh, level, begin, end, first, count);
        NEED(dev_src || !count);
        ctx->device().device_to_slots(slots.data() + first, count, dev_src);
    })
}
int fr_shard_finish(fr_ctx* ctx, fr_shard* sh, fr_ct* out, fr_match_stats* st) {
    FR_TRY({
        NEED(ctx && sh && out);
        *out = finish_output(ctx, sh->out, sh->plan.slot, false);
        if (st) *st = sh->stats;
    })
}
int fr_shard_free(fr_ctx* ctx, fr_shard* sh) {
    FR_TRY({
        NEED(ctx);
        delete sh;  // its plan waits for every lane first (Plan)
    })
}

// The same schedule without a device (CPU evaluators, tests): every content
// position of [0, n_chars) is taken as an encrypted radix character.
int fr_schedule_match(size_t n_chars, const char* pattern, size_t lo, size_t hi, int32_t lowering, int32_t engine,
                      int32_t grammar, int32_t multi_value, fr_job* jobs, size_t jobs_cap, size_t* n_jobs,
                      uint32_t* level_off, size_t level_cap, size_t* n_levels, int32_t* out3) {
    size_t n_parts = 0;
    return fr_schedule_match_parts(n_chars, pattern, lo, hi, lowering, engine, grammar, multi_value, 1, jobs, jobs_cap,
                                   n_jobs, level_off, level_cap, n_levels, out3, &n_parts);
}

int fr_schedule_match_parts(size_t n_chars, const char* pattern, size_t lo, size_t hi, int32_t lowering,
                            int32_t engine, int32_t grammar, int32_t multi_value, size_t max_parts, fr_job* jobs,
                            size_t jobs_cap, size_t* n_jobs, uint32_t* level_off, size_t level_cap, size_t* n_levels,
                            int32_t* outs3, size_t* n_parts) {
    FR_TRY({
        NEED(pattern && n_jobs && n_levels && outs3 && n_parts && lo <= hi);
        NEED(max_parts >= 1 && max_parts <= (size_t)MAX_FANIN);
        const Program prog =
            compile_match(MatchSpec{pattern, n_chars, lo, hi, engine, grammar, lowering, (int)max_parts}).prog;
        schedule_program(prog, n_chars, multi_value, jobs, jobs_cap, n_jobs, level_off, level_cap, n_levels, outs3,
                         n_parts);
    })
}

int fr_schedule_find(size_t n_chars, size_t m, size_t start_lo, size_t start_hi, int32_t starts, fr_job* jobs,
                     size_t jobs_cap, size_t* n_jobs, uint32_t* level_off, size_t level_cap, size_t* n_levels,
                     int32_t* outs3, size_t outs_cap, size_t* n_outs) {
    FR_TRY({
        NEED(n_jobs && n_levels && n_outs && outs3 && start_lo <= start_hi && (starts == 0 || starts == 1));
        NEED(outs_cap >= (starts ? start_hi - start_lo : 1));
        const Program prog = needle_program(MATCH_NEEDLE, n_chars, m, start_lo, start_hi, starts != 0);
        schedule_program(prog, n_chars, 1, jobs, jobs_cap, n_jobs, level_off, level_cap, n_levels, outs3, n_outs);
    })
}

int fr_schedule_find_clear(size_t n_chars, size_t m, size_t start_lo, size_t start_hi, int32_t starts, fr_job* jobs,
                           size_t jobs_cap, size_t* n_jobs, uint32_t* level_off, size_t level_cap, size_t* n_levels,
                           int32_t* outs3, size_t outs_cap, size_t* n_outs) {
    FR_TRY({
        NEED(n_jobs && n_levels && n_outs && outs3 && start_lo <= start_hi && (starts == 0 || starts == 1));
        NEED(outs_cap >= (starts ? start_hi - start_lo : 1));
        const Program prog = needle_program(MATCH_NEEDLE_CLEAR, n_chars, m, start_lo, start_hi, starts != 0);
        schedule_program(prog, n_chars, 1, jobs, jobs_cap, n_jobs, level_off, level_cap, n_levels, outs3, n_outs);
    })
}

int fr_schedule_scan_clear(size_t n_windows, size_t m, int32_t starts, fr_job* jobs, size_t jobs_cap, size_t* n_jobs,
                           uint32_t* level_off, size_t level_cap, size_t* n_levels, int32_t* outs3, size_t outs_cap,
                           size_t* n_outs) {
    FR_TRY({
        NEED(n_jobs && n_levels && n_outs && outs3 && (starts == 0 || starts == 1));
        NEED(n_windows <= ((size_t)1 << 24) && outs_cap >= (starts ? n_windows : 1));
        const Program prog = needle_program(MATCH_NEEDLE_WINDOWS, n_windows, m, 0, n_windows, starts != 0);
        // (the extract-sums read n_windows m bytes of compacted text)
        schedule_program(prog, n_windows * m, 1, jobs, jobs_cap, n_jobs, level_off, level_cap, n_levels, outs3, n_outs);
    })
}

int fr_schedule_find_clear_bytes(size_t n_chars, size_t m, size_t start_lo, size_t start_hi, int32_t starts,
                                 fr_job* jobs, size_t jobs_cap, size_t* n_jobs, uint32_t* level_off, size_t level_cap,
                                 size_t* n_levels, int32_t* outs3, size_t outs_cap, size_t* n_outs) {
    FR_TRY({
        NEED(n_jobs && n_levels && n_outs && outs3 && start_lo <= start_hi && (starts == 0 || starts == 1));
        NEED(outs_cap >= (starts ? start_hi - start_lo : 1));
        const Program prog = needle_program(MATCH_NEEDLE_CLEAR, n_chars, m, start_lo, start_hi, starts != 0, true);
        schedule_program(prog, n_chars, 1, jobs, jobs_cap, n_jobs, level_off, level_cap, n_levels, outs3, n_outs);
    })
}

int fr_schedule_scan_clear_bytes(size_t n_windows, size_t m, int32_t starts, fr_job* jobs, size_t jobs_cap,
                                 size_t* n_jobs, uint32_t* level_off, size_t level_cap, size_t* n_levels,
                                 int32_t* outs3, size_t outs_cap, size_t* n_outs) {
    FR_TRY({
        NEED(n_jobs && n_levels && n_outs && outs3 && (starts == 0 || starts == 1));
        NEED(n_windows <= ((size_t)1 << 24) && outs_cap >= (starts ? n_windows : 1));
        const Program prog = needle_program(MATCH_NEEDLE_WINDOWS, n_windows, m, 0, n_windows, starts != 0, true);
        schedule_program(prog, n_windows * m, 1, jobs, jobs_cap, n_jobs, level_off, level_cap, n_levels, outs3, n_outs);
    })
}

int fr_schedule_match_starts(size_t n_chars, const char* pattern, size_t lo, size_t hi, int32_t lowering,
                             int32_t engine, int32_t grammar, int32_t multi_value, fr_job* jobs, size_t jobs_cap,
                             size_t* n_jobs, uint32_t* level_off, size_t level_cap, size_t* n_levels, int32_t* outs3,
                             size_t outs_cap, size_t* n_starts) {
    FR_TRY({
        NEED(pattern && n_jobs && n_levels && n_starts && lo <= hi && (outs3 || lo == hi) && outs_cap >= hi - lo);
        const Program prog =
            compile_match_starts(MatchSpec{pattern, n_chars, lo, hi, engine, grammar, lowering, 1}).prog;
        schedule_program(prog, n_chars, multi_value, jobs, jobs_cap, n_jobs, level_off, level_cap, n_levels, outs3,
                         n_starts);
    })
}

}  // extern "C"
