// The level scheduler and the executor (internal; DESIGN.md §2.2 "Execution"): a PBS
// program becomes a Schedule of rotation jobs by dependency level, a Plan maps the
// schedule to arena slots, and launch_plan enqueues it level by level.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "device.h"
#include "fheregex.h"
#include "lower.h"

struct fr_ctx;

namespace fr {

// LUTs whose multi-value factor w_f has sum(d^2) <= this share rotations
constexpr int MV_MAX_NORM2 = 8;

// A PBS program whose negative sources refer to content blocks (input q = pos q:
// src = -(1 + q*4 + blk)) becomes a Schedule: its rotation jobs by dependency level,
// small-norm LUTs on the same linear combination merged into one multi-value job.
// Job references are abstract: in_slot[q] >= 0 is the output of program gate
// in_slot[q], in_slot[q] < 0 content block -1 - in_slot[q]; out_slot[f] is a program
// gate.  Trivial content blocks are folded into the offset.  Building a schedule
// validates every gate and allocates nothing; a host-only context builds the same
// schedule (fr_schedule_match) as the device plan, which maps the references to
// arena slots (compile_plan).
struct Schedule {
    std::vector<DevGate> jobs;      // levels concatenated
    std::vector<size_t> level_off;  // level l (0-based): jobs [level_off[l], level_off[l+1])
    // the program's extract-sums (level 0: before every job, and no job themselves); out_slot is
    // a program gate
    std::vector<DevSum> sums;
    size_t n_gates = 0;
    uint64_t levels = 0, max_width = 0;
};

// block(cb, &key, &triv): false if content block cb is trivial (its value in triv),
// else key identifies the block's ciphertext (the multi-value merge compares keys).
// A template parameter, not a std::function: it is called per content reference of
// every gate, twice, and the cold path of a match is this function.
// n_text: the clear content bytes an extract-sum's terms may refer to.
template <class BlockFn>
Schedule build_schedule(const std::vector<PGate>& gates, size_t n_content, bool multi_value, BlockFn&& block,
                        size_t n_text = 0) {
    // 1. validation: topological order, input range, fan-in, offsets
    std::vector<int> level(gates.size(), 0);
    int maxl = 0;
    std::vector<DevSum> sums;
    for (size_t g = 0; g < gates.size(); ++g) {
        const PGate& G = gates[g];
        if (G.kind == GATE_EXTRACT) {  // level 0 (the vector's initial value)
            if (!G.ins.empty() || G.terms.empty() || G.terms.size() > (size_t)SUM_MAX_TERMS)
                throw Error(FR_ERR_INVALID, "extract-sum: no inputs and 1..16 terms");
            DevSum d;
            std::memset(&d, 0, sizeof d);
            d.out_slot = (int32_t)g;
            for (const PTerm& t : G.terms) {
                if (t.sel < 0 || t.sel >= MAX_SELECTORS || t.pos < 0 || (size_t)t.pos >= n_text || t.half < 0 || t.half > 1)
                    throw Error(FR_ERR_INVALID, "extract-sum: term out of range");
                int32_t* w = d.term[d.n_terms++];
                w[0] = t.sel, w[1] = t.pos, w[2] = t.half;
            }
            sums.push_back(d);
            continue;
        }
        int nin = 0, off = G.offset;
        for (auto& in : G.ins) {
            if (in.src >= 0) {
                if ((size_t)in.src >= g) throw Error(FR_ERR_INVALID, "gate program is not topologically ordered");
                // a sum is not a boolean: only the AND it stands for may read it
                if (gates[in.src].kind == GATE_EXTRACT && (G.kind != GATE_SIGN || in.w != 1))
                    throw Error(FR_ERR_INVALID, "extract-sum read by other than a sign gate with weight 1");
                ++nin;
                continue;
            }
            const int cb = -in.src - 1;
            if ((size_t)(cb / 4) >= n_content) throw Error(FR_ERR_INVALID, "gate input out of range");
            int key = 0, triv = 0;
            if (block(cb, key, triv)) ++nin;
            else off += 2 * in.w * triv;
        }
        if (nin > 16) throw Error(FR_ERR_INVALID, "gate fan-in > 16");
        if (G.kind != GATE_SIGN && (off & 1)) throw Error(FR_ERR_INVALID, "LUT gate with a half-integral offset");
        if (G.kind == GATE_SELECT && (G.sel < 0 || G.sel >= MAX_SELECTORS))
            throw Error(FR_ERR_INVALID, "selector gate: index out of range");
        level[g] = gate_level(G, [&](int s) { return level[s]; });
        maxl = std::max(maxl, level[g]);
    }
    std::vector<std::vector<int>> by_level(maxl + 1);
    // (a level's selector gates first: their jobs are launched apart from the others, device.h)
    for (int sel = 1; sel >= 0; --sel)
        for (size_t g = 0; g < gates.size(); ++g)
            if ((gates[g].kind == GATE_SELECT) == (sel == 1)) by_level[level[g]].push_back((int)g);
    // 2. jobs, level by level
    Schedule S;
    S.sums = std::move(sums);
    S.n_gates = gates.size();
    S.level_off.push_back(0);
    for (int l = 1; l <= maxl; ++l) {
        const size_t first = S.jobs.size();
        // input signature -> open job index
        std::map<std::vector<int32_t>, size_t> open_job;
        for (int g : by_level[l]) {
            const PGate& G = gates[g];
            DevGate d;
            std::memset(&d, 0, sizeof d);
            int off = G.offset, nin = 0;
            std::vector<int32_t> sig;
            for (auto& in : G.ins) {
                int ref, key;
                if (in.src >= 0) {
                    ref = in.src;
                    key = in.src;
                } else {
                    const int cb = -in.src - 1;
                    int triv = 0;
                    if (!block(cb, key, triv)) {
                        off += 2 * in.w * triv;  // offsets are in units of Delta/2
                        continue;
                    }
                    ref = -1 - cb;
                    key = -1 - key;
                }
                d.in_slot[nin] = ref;
                d.in_w[nin] = in.w;
                sig.push_back(key);
                sig.push_back(in.w);
                ++nin;
            }
            d.n_in = nin;
            d.offset = off;
            if (G.kind == GATE_SIGN) {
                d.n_out = 1;
                d.direct = JOB_SIGN;
                d.out_slot[0] = g;
                S.jobs.push_back(d);
                continue;
            }
            if (G.kind == GATE_SELECT) {  // never merged: its table is the needle's, not the plan's
                d.n_out = 1;
                d.direct = JOB_ACC;
                set_acc_selector(d, (uint32_t)G.sel);
                d.out_slot[0] = g;
                S.jobs.push_back(d);
                continue;
            }
            const bool small = lut_w_norm2(G.lut) <= MV_MAX_NORM2;
            if (small && multi_value) {
                sig.push_back(nin);
                sig.push_back(off);
                auto it = open_job.find(sig);
                if (it != open_job.end() && S.jobs[it->second].n_out < MAX_OUT) {
                    DevGate& J = S.jobs[it->second];
                    std::memcpy(J.lut[J.n_out], G.lut, 16);
                    J.out_slot[J.n_out] = g;
                    J.n_out++;
                    J.direct = JOB_MULTI;
                    continue;
                }
                open_job[sig] = S.jobs.size();
            }
            std::memcpy(d.lut[0], G.lut, 16);
            d.n_out = 1;
            d.direct = JOB_DIRECT;
            d.out_slot[0] = g;
            S.jobs.push_back(d);
        }
        S.level_off.push_back(S.jobs.size());
        S.max_width = std::max<uint64_t>(S.max_width, S.jobs.size() - first);
    }
    S.levels = (uint64_t)maxl;
    return S;
}

// A device plan: the schedule with references mapped to arena slots (one slot per
// program gate).  A template plan (n_refs > 0) keeps its content inputs as references
// (in_slot = -1 - (4 pos + block)) that a content map bound per call resolves
// (Device::bind_content), so one plan serves every content of the same shape.
// A plan owns its slots and its device batch and is move-only.  The one rule of release: a
// resident plan (d_gates: a cached match, a shard plan) is replayed on every lane, so nothing
// of it goes while a level of it may be in flight -- its destructor synchronises every lane
// first.  A plan without a device batch runs once, on lane 0: its slots go back in stream
// order, without a wait.
struct Plan {
    std::vector<DevGate> gates;     // levels concatenated
    std::vector<size_t> level_off;  // level l (0-based): gates [level_off[l], level_off[l+1])
    Slots slot;                     // output slot per program gate
    uint64_t pbs = 0, rotations = 0, levels = 0, max_width = 0;
    size_t n_refs = 0;              // template plan: content references (4 per position)
    gpu::DevBuf<DevGate> d_gates;   // device-resident copy (cached plans)
    // extract-sums (a find over clear content): launched before level 1 into the plan's own
    // slots, over the needle and the content bytes the call bound to its lane; their
    // device-resident copy goes with d_gates, under the same rule
    std::vector<DevSum> sums;
    gpu::DevBuf<DevSum> d_sums;

    Plan() = default;
    Plan(Plan&&) = default;
    Plan& operator=(Plan&&) = default;  // (onto a plan that is not resident)
    ~Plan() {
        if (!d_gates) return;
        try {
            slot.arena()->sync();
        } catch (...) {  // (the members release all the same)
        }
    }
};

// n_text: the clear content bytes the program's extract-sums may refer to
Plan compile_plan(fr_ctx* ctx, const std::vector<PGate>& gates, const std::vector<fr_ct>& inputs,
                  bool content_refs = false, size_t n_text = 0);
// enqueue every level of a plan (async on the device stream)
void launch_plan(Device& dev, const Plan& P);
void add_plan_stats(const Plan& P, fr_match_stats* st);

// Runs a program and returns one slot per gate.
Slots execute_gates(fr_ctx* ctx, const std::vector<PGate>& gates, const std::vector<fr_ct>& inputs, fr_match_stats* st);
// out = offset * Delta/2 + w * arena[slot] in a fresh slot (a linear op, no bootstrap), enqueued
Slots linear_to_new_slot(Device& dev, int slot, int w, int offset);
// result handle of a program: boolean o.cst + o.w * gate slot (a linear
// op, no bootstrap), or trivial.  take_slot: the output gate's slot becomes the
// result's (else the result is a fresh slot and `slots` stay untouched).  Async:
// the caller synchronises the stream before handing the result out.
fr_ct make_output(fr_ctx* ctx, ProgOut o, Slots& slots, bool take_slot);
// the same, synchronised; take_slot also frees the other slots
fr_ct finish_output(fr_ctx* ctx, ProgOut o, Slots& slots, bool take_slot);
fr_ct run_program(fr_ctx* ctx, const Program& prog, const std::vector<fr_ct>& inputs, fr_match_stats* st);

}  // namespace fr
