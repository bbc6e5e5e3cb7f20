// The executor (plan.h): schedules compiled to arena slots, launched level by level,
// and the result handle of a program.
#include "plan.h"

#include "ctx.h"

namespace fr {

Plan compile_plan(fr_ctx* ctx, const std::vector<PGate>& gates, const std::vector<fr_ct>& inputs, bool content_refs,
                  size_t n_text) {
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
    }, n_text);
    Plan P;
    P.slot = Slots(dev, gates.size());
    P.gates = std::move(S.jobs);
    for (DevGate& d : P.gates) {
        for (int q = 0; q < d.n_in; ++q)
            d.in_slot[q] = d.in_slot[q] >= 0 ? P.slot[d.in_slot[q]]
                           : content_refs   ? d.in_slot[q]
                                            : block_slot(-1 - d.in_slot[q]).slot;
        for (int f = 0; f < d.n_out; ++f) d.out_slot[f] = P.slot[d.out_slot[f]];
    }
    P.sums = std::move(S.sums);
    for (DevSum& d : P.sums) d.out_slot = P.slot[d.out_slot];
    P.n_refs = content_refs ? 4 * inputs.size() : 0;
    P.level_off = std::move(S.level_off);
    P.pbs = gates.size() - P.sums.size();  // (an extract-sum is no bootstrap)
    P.rotations = P.gates.size();
    P.levels = S.levels;
    P.max_width = S.max_width;
    return P;
}

void launch_plan(Device& dev, const Plan& P) {
    if (P.d_sums) dev.run_sums_resident(P.d_sums.get(), P.sums.data(), P.sums.size());
    else dev.run_sums(P.sums.data(), P.sums.size());
    for (size_t l = 0; l + 1 < P.level_off.size(); ++l) {
        const size_t a = P.level_off[l], n = P.level_off[l + 1] - a;
        if (P.d_gates) dev.run_level_resident(P.d_gates.get() + a, P.gates.data() + a, n, P.n_refs);
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

Slots execute_gates(fr_ctx* ctx, const std::vector<PGate>& gates, const std::vector<fr_ct>& inputs, fr_match_stats* st) {
    Plan P = compile_plan(ctx, gates, inputs);
    launch_plan(ctx->device(), P);
    add_plan_stats(P, st);
    return std::move(P.slot);
}

Slots linear_to_new_slot(Device& dev, int slot, int w, int offset) {
    Slots out(dev, 1);
    DevGate d = affine_gate(slot, w, 0);
    d.offset = offset;  // (units of Delta / 2)
    d.out_slot[0] = out[0];
    dev.run_linear(d);
    return out;
}

fr_ct make_output(fr_ctx* ctx, ProgOut o, Slots& slots, bool take_slot) {
    if (o.gate < 0) return ctx->new_bool(-1, (uint8_t)o.cst);
    ctx->reserve_handles(1);  // new_bool cannot fail once a slot has left its owner
    if (take_slot && o.w == 1 && o.cst == 0) return ctx->new_bool(slots.take(o.gate));
    return ctx->new_bool(linear_to_new_slot(ctx->device(), slots[o.gate], o.w, 2 * o.cst).take(0));
}
fr_ct finish_output(fr_ctx* ctx, ProgOut o, Slots& slots, bool take_slot) {
    const fr_ct h = make_output(ctx, o, slots, take_slot);
    if (take_slot) slots.reset();
    ctx->device().sync();
    return h;
}

fr_ct run_program(fr_ctx* ctx, const Program& prog, const std::vector<fr_ct>& inputs, fr_match_stats* st) {
    Slots slots = execute_gates(ctx, prog.gates, inputs, st);
    return finish_output(ctx, prog.outs[0], slots, true);
}

}  // namespace fr
