// The arena-slot owner (csrc/owned.h: SlotsOf) against a counting fake arena, without a GPU:
//   g++ -std=c++17 -I fhe-regex_amd/csrc tests/slot_owner_check.cpp -o slot_owner_check && ./slot_owner_check
// The fake records the live slots and aborts on a double free or on a free of a slot it never
// gave out; every case ends with the arena's books checked.  tests/test_host.py builds and runs
// it; built with -fsanitize=address,undefined it is the owner's sanitizer run.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>

#include "owned.h"

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #x); \
            std::abort();                                                \
        }                                                                \
    } while (0)

struct FakeArena {
    std::set<int> live;
    std::vector<int> free_list, freed;  // freed: every free, in order
    int next = 0, allocs = 0, fail_at = 0;  // fail_at: the allocation (1-based) that throws
    int alloc_slot() {
        if (++allocs == fail_at) throw std::runtime_error("arena: out of memory");
        int s;
        if (!free_list.empty()) {
            s = free_list.back();
            free_list.pop_back();
        } else {
            s = next++;
        }
        CHECK(live.insert(s).second);
        return s;
    }
    void free_slot(int s) {
        CHECK(live.erase(s) == 1);  // a double free, or a slot never given out
        free_list.push_back(s);
        freed.push_back(s);
    }
};
using Slots = fr::gpu::SlotsOf<FakeArena>;

static void alloc_then_destruction() {
    FakeArena a;
    {
        Slots s(a, 5);
        CHECK(s.size() == 5 && a.live.size() == 5 && s.arena() == &a);
        for (int i = 0; i < 5; ++i) CHECK(s[i] == i && s.data()[i] == i);  // ascending
    }
    CHECK(a.live.empty() && a.freed == (std::vector<int>{0, 1, 2, 3, 4}));  // ascending
    Slots none(a);
    CHECK(none.size() == 0);
    Slots unbound;  // no arena: nothing to give back
}

static void failed_alloc_leaves_nothing() {
    for (int i = 1; i <= 4; ++i) {
        FakeArena a;
        a.fail_at = i;
        Slots s(a);
        bool threw = false;
        try {
            s.alloc(4);
        } catch (const std::runtime_error&) {
            threw = true;
        }
        CHECK(threw && s.size() == 0 && a.live.empty() && (int)a.freed.size() == i - 1);
        s.alloc(3);  // the owner is usable afterwards
        CHECK(s.size() == 3 && a.live.size() == 3);
    }
    FakeArena a;
    a.fail_at = 2;
    bool threw = false;
    try {
        Slots s(a, 3);  // the constructor allocates the same way
    } catch (const std::runtime_error&) {
        threw = true;
    }
    CHECK(threw && a.live.empty() && a.freed.size() == 1);
}

static void alloc_replaces() {
    FakeArena a;
    Slots s(a, 2);
    s.alloc(3);  // the previous slots go first
    CHECK(s.size() == 3 && a.live.size() == 3 && a.freed == (std::vector<int>{0, 1}));
    s.reset();
    CHECK(s.size() == 0 && a.live.empty());
    s.reset();
}

static void take_keeps_one() {
    FakeArena a;
    int kept;
    {
        Slots s(a, 4);
        kept = s.take(2);
        CHECK(kept == 2 && s[2] == -1 && s.size() == 4);
    }
    CHECK(a.live == std::set<int>{kept} && a.freed == (std::vector<int>{0, 1, 3}));
    a.free_slot(kept);
}

static void release_frees_none() {
    FakeArena a;
    std::vector<int> v;
    {
        Slots s(a, 3);
        v = s.release();
        CHECK(s.size() == 0);
    }
    CHECK(v == (std::vector<int>{0, 1, 2}) && a.live.size() == 3 && a.freed.empty());
    for (int x : v) a.free_slot(x);
}

static void move_construction() {
    FakeArena a;
    {
        Slots s(a, 3);
        Slots t(std::move(s));
        CHECK(s.size() == 0 && t.size() == 3 && t.arena() == &a && a.live.size() == 3);
    }
    CHECK(a.live.empty() && a.freed.size() == 3);
}

static void move_assignment_frees_the_target_first() {
    FakeArena a, b;
    {
        Slots s(a, 2), t(b, 3);
        t = std::move(s);
        CHECK(b.live.empty() && b.freed.size() == 3);  // the target's own slots, to its own arena
        CHECK(s.size() == 0 && t.size() == 2 && t.arena() == &a && a.live.size() == 2 && a.freed.empty());
    }
    CHECK(a.live.empty() && a.freed.size() == 2);
}

static void self_move() {
    FakeArena a;
    {
        Slots s(a, 3);
        Slots& r = s;
        s = std::move(r);
        CHECK(s.size() == 3 && a.live.size() == 3 && a.freed.empty());
    }
    CHECK(a.live.empty());
}

static Slots two_then_throw(FakeArena& a) {
    Slots s(a, 2);
    Slots more(a, 2);
    throw std::runtime_error("a launch failed");
    return s;
}
static void unwinding() {
    FakeArena a;
    bool threw = false;
    try {
        Slots outer(a, 1);
        Slots got = two_then_throw(a);
        CHECK(false);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    CHECK(threw && a.live.empty() && a.freed.size() == 5);
}

int main() {
    alloc_then_destruction();
    failed_alloc_leaves_nothing();
    alloc_replaces();
    take_keeps_one();
    release_frees_none();
    move_construction();
    move_assignment_frees_the_target_first();
    self_move();
    unwinding();
    std::puts("slot owner ok: 9 cases");
    return 0;
}
