// The executor (plan.h): schedules compiled to arena slots, launched level by level,
// and the result handle of a program.
#include "plan.h"

#include "ctx.h"

namespace fr {

void free_plan_slots(Device& dev, std::vector<int>& slot) {
    for (int& s : slot)
        if (s >= 0) dev.free_slot(s), s = -1;
}

void release_plan(Device& dev, Plan& P) {
    dev.sync();  // no level of this plan may still be in flight (every match ends synchronised)
    free_plan_slots(dev, P.slot);
    dev.free_gates(P.d_gates);
    P.d_gates = nullptr;
}

Plan compile_plan(fr_ctx* ctx, const std::vector<PGate>& gates, const std::vector<fr_ct>& inputs, bool content_refs) {
    Device& dev = ctx->keyed_device();
    auto block_slot = [&](int cb) -> const Block& { return ctx->get(inputs[(size_t)(cb / 4)]).b[cb % 4]; };
    Schedule S = build_schedule(gates, inputs.size(), ctx->multi_value, [&](int cb, int& key, int& triv) {
        const Block& b = block_slot(cb);
        if (b.slot < 0) {
            triv = (int)b.triv;
            return false;
        }
        key = b.slot;
        return true;
    });
    Plan P;
    P.slot.assign(gates.size(), -1);
    struct Guard {
        Device& dev;
        std::vector<int>& slot;
        bool armed = true;
        ~Guard() {
            if (armed) free_plan_slots(dev, slot);
        }
    } guard{dev, P.slot};
    for (size_t g = 0; g < gates.size(); ++g) P.slot[g] = dev.alloc_slot();
    P.gates = std::move(S.jobs);
    for (DevGate& d : P.gates) {
        for (int q = 0; q < d.n_in; ++q)
            d.in_slot[q] = d.in_slot[q] >= 0 ? P.slot[d.in_slot[q]]
                           : content_refs   ? d.in_slot[q]
                                            : block_slot(-1 - d.in_slot[q]).slot;
        for (int f = 0; f < d.n_out; ++f) d.out_slot[f] = P.slot[d.out_slot[f]];
    }
    P.n_refs = content_refs ? 4 * inputs.size() : 0;
    P.level_off = std::move(S.level_off);
    P.pbs = gates.size();
    P.rotations = P.gates.size();
    P.levels = S.levels;
    P.max_width = S.max_width;
    guard.armed = false;
    return P;
}

void launch_plan(Device& dev, const Plan& P) {
    for (size_t l = 0; l + 1 < P.level_off.size(); ++l) {
        const size_t a = P.level_off[l], n = P.level_off[l + 1] - a;
        if (P.d_gates) dev.run_level_resident(P.d_gates + a, P.gates.data() + a, n, P.n_refs);
        else dev.run_level(P.gates.data() + a, n);
    }
}

void add_plan_stats(const Plan& P, fr_match_stats* st) {
    if (!st) return;
    st->pbs += P.pbs;
    st->blind_rotations += P.rotations;
    st->levels += P.levels;
    st->max_level_width = std::max<uint64_t>(st->max_level_width, P.max_width);
}

std::vector<int> execute_gates(fr_ctx* ctx, const std::vector<PGate>& gates, const std::vector<fr_ct>& inputs,
                               fr_match_stats* st) {
    Plan P = compile_plan(ctx, gates, inputs);
    launch_plan(ctx->device(), P);
    add_plan_stats(P, st);
    return std::move(P.slot);
}

int linear_to_new_slot(Device& dev, int slot, int w, int offset) {
    DevGate d;
    std::memset(&d, 0, sizeof d);
    d.n_in = 1;
    d.in_slot[0] = slot;
    d.in_w[0] = w;
    d.offset = offset;
    d.out_slot[0] = dev.alloc_slot();
    dev.run_linear(d);
    return d.out_slot[0];
}

fr_ct make_output(fr_ctx* ctx, ProgOut o, std::vector<int>& slots, bool take_slot) {
    if (o.gate < 0) return ctx->new_bool(-1, (uint8_t)o.cst);
    if (take_slot && o.w == 1 && o.cst == 0) {
        const int s = slots[o.gate];
        slots[o.gate] = -1;
        return ctx->new_bool(s);
    }
    return ctx->new_bool(linear_to_new_slot(ctx->device(), slots[o.gate], o.w, 2 * o.cst));
}
fr_ct finish_output(fr_ctx* ctx, ProgOut o, std::vector<int>& slots, bool take_slot) {
    const fr_ct h = make_output(ctx, o, slots, take_slot);
    if (take_slot) free_plan_slots(ctx->device(), slots);
    ctx->device().sync();
    return h;
}

fr_ct run_program(fr_ctx* ctx, const Program& prog, const std::vector<fr_ct>& inputs, fr_match_stats* st) {
    std::vector<int> slots = execute_gates(ctx, prog.gates, inputs, st);
    return finish_output(ctx, ProgOut{prog.out_gate, prog.out_w, prog.out_const}, slots, true);
}

}  // namespace fr
