// The context behind the C ABI's opaque fr_ctx (internal): parameters, keys, ciphertext
// handles, the plan cache's storage, and the error boundary every entry point goes through.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device.h"
#include "fheregex.h"
#include "keys.h"
#include "plan.h"
#include "regex.h"
#include "wire.h"

namespace fr {

// PARAM_MESSAGE_2_CARRY_2 (ciphertext.rs:1): 2-bit message, 2-bit carry per block
constexpr uint64_t MESSAGE_MODULUS = 4, CARRY_MODULUS = 4;

struct Block {
    int slot = -1;     // -1: trivial block
    uint8_t triv = 0;  // value of a trivial block (message, < 16)
};
struct HandleRec {
    bool live = false;
    bool is_bool = false;  // block 0 carries 0/1, blocks 1..3 trivial zero
    Block b[4];
};

static inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// One cached match plan (match.cpp: the plan cache)
struct CachedMatch {
    std::string key;           // match_key: every numeric field first, the pattern last
    size_t parts = 1;          // fr_has_match_parts' max_parts (also in the key)
    int lane = 0;              // lane whose plan copy this is (0: lane 0; also in the key)
    std::vector<int32_t> sig;  // canonical content shape (content_signature)
    Plan plan;
    size_t n_gates = 0;        // program gates of one match (copy m's gates start at m * n_gates)
    std::vector<ProgOut> outs;  // one match's outputs (its parts, fr_has_match_parts)
    Recorded rec;              // the recording's counters
    uint64_t last_use = 0;
};

}  // namespace fr

struct fr_plan_cache {
    std::vector<std::unique_ptr<fr::CachedMatch>> entries;
    size_t capacity = 8;
    size_t slot_cap = (size_t)1 << 18;  // intermediate slots held by all cached plans
    size_t slots_held = 0;
    uint64_t clock = 0, hits = 0, misses = 0;

    fr_plan_cache() {
        if (const char* ev = std::getenv("FR_PLAN_CACHE")) capacity = (size_t)std::max(0, std::atoi(ev));
        if (const char* ev = std::getenv("FR_PLAN_CACHE_SLOTS")) slot_cap = (size_t)std::max(0L, std::atol(ev));
    }
};

struct fr_ctx {
    fr::Params p;
    std::unique_ptr<fr::Device> dev;
    fr::ClientKey ck;
    bool has_ck = false;
    std::vector<uint64_t> ksk, bsk;
    bool has_sk = false;
    std::vector<fr::HandleRec> handles;
    std::vector<uint32_t> free_handles;
    int lowering = FR_LOWER_THRESHOLD;
    int engine = FR_ENGINE_AUTO;
    int grammar = FR_GRAMMAR_REFERENCE;
    int keygen = FR_KEYGEN_AUTO;
    bool sk_on_device = false;  // server key generated on the device (export downloads it)
    bool sk_compact = false;    // the server key is in compact form (keys.h): mask_key expands its masks
    fr::RngKey mask_key{};      // public by design
    // packing key (keys.h), optional: on a device context it lives on the device (the torus rows
    // stay there for export); a host-only context keeps the rows here
    std::vector<uint64_t> pksk;
    bool has_pk = false;
    bool pk_compact = false;   // the packing key is in compact form (keys.h): pk_mask_key expands its masks
    fr::RngKey pk_mask_key{};  // public by design
    bool multi_value = true;  // merge same-input small-norm LUTs into one blind rotation
    bool async_match = true;  // has_match returns once its launches are enqueued (fr_set_async)
    uint64_t next_lane = 0;   // fr_set_lanes: consecutive asynchronous matches round-robin over the lanes
    uint64_t scan_classes = 0, scan_padded = 0;  // the last scan's distinct windows, and their padded count (fr_scan_classes)
    fr_plan_cache plans;  // after dev: the cached plans go while the device is alive (Plan, plan.h)
    // content_signature scratch: canonical id of an arena slot, valid while sig_gen[slot] == gen
    std::vector<int32_t> sig_id;
    std::vector<uint32_t> sig_gen;
    uint32_t gen = 0;

    fr::Device& device() {
        if (!dev) throw fr::Error(FR_ERR_NO_DEVICE, "host-only context: no HIP device");
        return *dev;
    }
    // the device, once it holds a server key (what every bootstrap needs)
    fr::Device& keyed_device() {
        fr::Device& d = device();
        if (!has_sk || !d.has_keys()) throw fr::Error(FR_ERR_NO_KEY, "server key not generated");
        return d;
    }
    // every pack refuses here, before anything is launched
    void need_packing_key() const {
        if (!has_pk)
            throw fr::Error(FR_ERR_INVALID, "packing needs a packing key (fr_gen_packing_key, fr_load_packing_key)");
    }
    fr_ct new_handle(const fr::HandleRec& r) {
        uint32_t h;
        if (!free_handles.empty()) {
            h = free_handles.back();
            free_handles.pop_back();
            handles[h] = r;
        } else {
            h = (uint32_t)handles.size();
            handles.push_back(r);
        }
        handles[h].live = true;
        return h;
    }
    // a boolean handle: block 0 in arena slot `slot`, or (slot < 0) the trivial value triv
    fr_ct new_bool(int slot, uint8_t triv = 0) {
        fr::HandleRec r;
        r.is_bool = true;
        r.b[0].slot = slot;
        r.b[0].triv = triv;
        return new_handle(r);
    }
    // room for n more handles, so that new_handle cannot fail (grown geometrically)
    void reserve_handles(size_t n) {
        const size_t need = handles.size() + n;
        if (need > handles.capacity()) handles.reserve(std::max(need, 2 * handles.capacity()));
    }
    // Handles over owned slots: a radix character per four consecutive slots, or a boolean per
    // slot.  The table is reserved first, so the slots change hands only once nothing can fail.
    void adopt(fr::Slots&& slots, bool radix, fr_ct* out) {
        const size_t per = radix ? 4 : 1, n = slots.size() / per;
        reserve_handles(n);
        const std::vector<int> s = slots.release();
        for (size_t i = 0; i < n; ++i) {
            fr::HandleRec r;
            r.is_bool = !radix;
            for (size_t b = 0; b < per; ++b) r.b[b].slot = s[per * i + b];
            out[i] = new_handle(r);
        }
    }
    fr::HandleRec& get(fr_ct h) {
        if (h >= handles.size() || !handles[h].live) throw fr::Error(FR_ERR_INVALID, "invalid ciphertext handle");
        return handles[h];
    }
    void release(fr_ct h) {
        fr::HandleRec& r = get(h);
        for (auto& b : r.b)
            if (b.slot >= 0 && dev) dev->free_slot(b.slot);
        r.live = false;
        free_handles.push_back(h);
    }
};

namespace fr {

// the pack row of a boolean handle: its slot, or its trivial value; `not_bool` is the caller's
// refusal of any other handle
inline DevGate bool_gate(const HandleRec& h, const char* not_bool) {
    if (!h.is_bool) throw Error(FR_ERR_INVALID, not_bool);
    return affine_gate(h.b[0].slot, 1, h.b[0].slot >= 0 ? 0 : h.b[0].triv & 1);
}
// n results packed under the packing key on the current lane (capi_pack.cpp): result j is
// rows[map[j]] (-1: the constant 0), or rows[j] without a map (n_rows == n) -- the (k+1) N words
// of the packed GLWE, or (v) the compact blob's rounded values.  A host-only context packs
// trivial rows, unmapped.
void pack_rows(fr_ctx* ctx, const DevGate* rows, size_t n_rows, const int32_t* map, size_t n, uint64_t* words,
               uint16_t* v);
// the same as the wire blob at buf (compact: FRCPRES1, else FRPKRES1); returns its bytes.  No row
// at all is the packing of n constants 0: all-zero words, nothing launched.
size_t pack_to_blob(fr_ctx* ctx, const DevGate* rows, size_t n_rows, const int32_t* map, size_t n, bool compact,
                    uint8_t* buf);

}  // namespace fr

// a needle uploaded to a device context (private search): its selectors and the (k, N) they are for
struct fr_needle {
    fr::DevNeedle dev;
    int k = 0, N = 0;
};

#define FR_TRY(...)                                   \
    try {                                             \
        __VA_ARGS__;                                       \
        return FR_OK;                                 \
    } catch (const fr::Error& e) {                    \
        fr::set_last_error(e.what());                 \
        return e.code;                                \
    } catch (const std::bad_alloc&) {                 \
        fr::set_last_error("out of memory");          \
        return FR_ERR_OOM;                            \
    } catch (const std::exception& e) {               \
        fr::set_last_error(e.what());                 \
        return FR_ERR_INVALID;                        \
    } catch (...) {                                   \
        fr::set_last_error("unknown error");          \
        return FR_ERR_INVALID;                        \
    }

#define NEED(x)                                                               \
    do {                                                                      \
        if (!(x)) throw fr::Error(FR_ERR_INVALID, "invalid argument: " #x);   \
    } while (0)

// The size query of an entry that writes `need` bytes: *written = need either way; true if the
// call only asked (no buffer) and is done, else the buffer holds them.
inline bool answer_size(size_t* written, size_t need, const void* buf, size_t cap) {
    *written = need;
    if (!buf) return true;
    NEED(cap >= need);
    return false;
}
