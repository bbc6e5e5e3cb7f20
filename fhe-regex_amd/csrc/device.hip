// The Device host class (HIP, gfx950): context construction, streams and lanes, the arena
// of big-LWE slots and its packed slot copies, gate staging and validation, running a
// dependency level (keyswitch + blind rotation), timers, and the single-stage entry points
// of the parity tests.  The kernels of a level live with the methods that launch them:
// rns_br.hip (RNS blind rotation), fft_br.hip (FFT blind rotation), keyswitch.hip, and
// keygen.hip (server-key generation, encryption).
//
//   k_slots_to_buf, k_slots_to_buf_arg, k_buf_to_slots : packed copies between arena slots
//                         and a device buffer of the caller
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <sstream>

#include "device_impl.h"

namespace fr {

static bool supported(const Params& p) {
    if (p.ring == FR_RING_FFT) return (p.N == 2048 && p.k == 1) || (p.N == 1024 && p.k == 2);
    return (p.N == 2048 && p.k == 1) || (p.N == 1024 && p.k == 2) || (p.N == 1024 && p.k == 1);
}

Device::Device(const Params& p, int device) : p_(p), dev_(device) {
    if (!supported(p)) throw Error(FR_ERR_INVALID, "device: unsupported (k, N)");
    if (p.ks_base_log != 3 || p.ks_level != 5 || p.pbs_base_log != 23 || p.pbs_level != 1)
        throw Error(FR_ERR_INVALID, "device: only KS 2^3x5 and PBS 2^23x1 are compiled");
    if (p.n > 1024) throw Error(FR_ERR_INVALID, "device: n > 1024");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= device || device < 0)
        throw Error(FR_ERR_NO_DEVICE, "no usable HIP device " + std::to_string(device));
    HIP_CHECK(hipSetDevice(device));
    hipStream_t s;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    stream_ = s;
    for (auto& e : ev_) {
        hipEvent_t ev;
        HIP_CHECK(hipEventCreate(&ev));
        e = ev;
    }
    for (auto* evs : {&stage_ev_, &cmap_ev_})
        for (auto& e : *evs) {
            hipEvent_t ev;
            HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            HIP_CHECK(hipEventRecord(ev, s));  // complete before first use
            e = ev;
        }
    init_rns();  // (an FFT-ring context too: twiddles and kernel attributes)
    init_ks();
    if (const char* ev = std::getenv("FR_TIMER_CHAIN")) timer_chain_ = std::atoi(ev) != 0;
    if (p.ring == FR_RING_FFT) init_fft();
    ensure_arena(1024);
    ensure_batch(1024);
}

Device::~Device() {
    (void)hipSetDevice(dev_);
    if (lane_ != 0) leave_lane();
    for (auto& l : lanes_) {
        if (l.stream) (void)hipStreamSynchronize((hipStream_t)l.stream);
        free_lane(l);
    }
    lanes_.clear();
    if (main_ev_) (void)hipEventDestroy((hipEvent_t)main_ev_);
    if (stream_) (void)hipStreamSynchronize((hipStream_t)stream_);
    (void)hipFree(d_ksk_);
    (void)hipFree(d_tbsk_);
    (void)hipFree(d_kl_);
    (void)hipFree(d_dig_);
    free_rns();
    free_fft();
    (void)hipFree(d_arena_);
    (void)hipFree(d_gates_);
    (void)hipFree(d_ks_);
    (void)hipFree(d_slot_list_);
    (void)hipFree(d_xstage_);
    for (auto* h : h_xstage_)
        if (h) (void)hipHostFree(h);
    for (auto* e : xstage_ev_)
        if (e) (void)hipEventDestroy((hipEvent_t)e);
    for (auto* h : h_stage_)
        if (h) (void)hipHostFree(h);
    for (auto* e : stage_ev_)
        if (e) (void)hipEventDestroy((hipEvent_t)e);
    for (auto* e : cmap_ev_)
        if (e) (void)hipEventDestroy((hipEvent_t)e);
    (void)hipFree(d_cmap_);
    for (auto* h : h_cmap_)
        if (h) (void)hipHostFree(h);
    for (auto& t : pending_)
        for (auto* e : t.ev) (void)hipEventDestroy((hipEvent_t)e);
    for (auto* e : event_pool_) (void)hipEventDestroy((hipEvent_t)e);
    for (auto e : ev_)
        if (e) (void)hipEventDestroy((hipEvent_t)e);
    if (stream_) (void)hipStreamDestroy((hipStream_t)stream_);
}

// ---------------------------------------------------------------- lanes
void Device::swap_lane(LaneState& l) {
    std::swap(stream_, l.stream);
    std::swap(d_ks_, l.d_ks);
    std::swap(batch_cap_, l.batch_cap);
    std::swap(d_dig_, l.d_dig);
    std::swap(dig_cap_, l.dig_cap);
    std::swap(d_cmap_, l.d_cmap);
    std::swap(h_cmap_, l.h_cmap);
    std::swap(cmap_ev_, l.cmap_ev);
    std::swap(cmap_cap_, l.cmap_cap);
    std::swap(cmap_n_, l.cmap_n);
    std::swap(cmap_stage_, l.cmap_stage);
}
void Device::free_lane(LaneState& l) {
    (void)hipFree(l.d_ks);
    (void)hipFree(l.d_dig);
    (void)hipFree(l.d_cmap);
    for (auto* h : l.h_cmap)
        if (h) (void)hipHostFree(h);
    for (auto* e : l.cmap_ev)
        if (e) (void)hipEventDestroy((hipEvent_t)e);
    if (l.done_ev) (void)hipEventDestroy((hipEvent_t)l.done_ev);
    if (l.stream) (void)hipStreamDestroy((hipStream_t)l.stream);
    l = LaneState{};
}
void Device::set_lanes(int n) {
    if (n < 1 || n > 8) throw Error(FR_ERR_INVALID, "lanes: 1..8");
    if (lane_ != 0) throw Error(FR_ERR_INVALID, "lanes: changed inside a lane");
    sync_all();
    // n >= 2: n lanes besides lane 0 (matches go to them only: a match on lane 0 would wait
    // for the other lanes at its first launch)
    const int extra = n >= 2 ? n : 0;
    while ((int)lanes_.size() > extra) {
        free_lane(lanes_.back());
        lanes_.pop_back();
    }
    if (!main_ev_ && extra) {
        hipEvent_t ev;
        HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        main_ev_ = ev;
    }
    while ((int)lanes_.size() < extra) {
        LaneState l;
        hipStream_t st;
        HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        l.stream = st;
        for (auto*& e : l.cmap_ev) {
            hipEvent_t ev;
            HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            HIP_CHECK(hipEventRecord(ev, st));  // complete before first use
            e = ev;
        }
        hipEvent_t dv;
        HIP_CHECK(hipEventCreateWithFlags(&dv, hipEventDisableTiming));
        l.done_ev = dv;
        lanes_.push_back(l);
        // the lane's keyswitch scratch at the main lane's size (ensure_batch on entry grows it)
        const int i = (int)lanes_.size();
        enter_lane(i);
        ensure_batch(1024);
        leave_lane();
    }
}
void Device::enter_lane(int i) {
    if (lane_ != 0) throw Error(FR_ERR_INVALID, "lanes: already inside a lane");
    if (i <= 0) return;
    if (i > (int)lanes_.size()) throw Error(FR_ERR_INVALID, "lanes: no such lane");
    // the lane waits for lane 0's own work so far -- not for the other lanes (no join here:
    // that would chain every lane behind the previous one); lane 0 waited for the lanes at
    // its last operation, so their results that operation consumed are covered too
    HIP_CHECK(hipEventRecord((hipEvent_t)main_ev_, (hipStream_t)stream_));
    swap_lane(lanes_[i - 1]);
    lane_ = i;
    HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream_, (hipEvent_t)main_ev_, 0));
}
void Device::leave_lane() {
    if (lane_ == 0) return;
    LaneState& l = lanes_[lane_ - 1];
    HIP_CHECK(hipEventRecord((hipEvent_t)l.done_ev, (hipStream_t)stream_));
    swap_lane(l);
    l.pending = true;
    lanes_pending_ = true;
    lanes_unsynced_ = true;
    lane_ = 0;
}
void Device::join_lanes() {
    if (!lanes_pending_ || lane_ != 0) return;
    for (auto& l : lanes_)
        if (l.pending) {
            HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream_, (hipEvent_t)l.done_ev, 0));
            l.pending = false;
        }
    lanes_pending_ = false;
}
void* Device::cur_stream() {
    if (lane_ == 0 && lanes_pending_) join_lanes();
    return stream_;
}
void Device::sync_all() {
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_));
    for (auto& l : lanes_)
        if (l.stream) HIP_CHECK(hipStreamSynchronize((hipStream_t)l.stream));
    if (lane_ == 0) {
        for (auto& l : lanes_) l.pending = false;
        lanes_pending_ = false;
    }
    lanes_unsynced_ = false;
    free_slots_.insert(free_slots_.end(), deferred_free_.begin(), deferred_free_.end());
    deferred_free_.clear();
}

std::string Device::info() const {
    hipDeviceProp_t prop;
    (void)hipGetDeviceProperties(&prop, dev_);
    std::ostringstream o;
    o << prop.name << " " << prop.gcnArchName << " CUs=" << prop.multiProcessorCount;
    if (p_.ring == FR_RING_FFT) o << " ring=fft E=" << fft_e_ << " latency<=" << fft_small_;
    else o << " ring=rns E=" << e_;
    return o.str();
}

void Device::ensure_arena(size_t slots) {
    if (slots <= arena_cap_) return;
    size_t cap = arena_cap_ ? arena_cap_ : 1024;
    while (cap < slots) cap *= 2;
    uint64_t* nb = nullptr;
    HIP_CHECK(hipMalloc(&nb, (size_t)8 * p_.slot_stride() * cap));
    if (d_arena_) {
        sync_all();  // no launch of any lane may still use the old arena
        HIP_CHECK(hipMemcpyAsync(nb, d_arena_, (size_t)8 * p_.slot_stride() * arena_cap_, hipMemcpyDeviceToDevice, STREAM));
        HIP_CHECK(hipStreamSynchronize(STREAM));
        HIP_CHECK(hipFree(d_arena_));
    }
    d_arena_ = nb;
    arena_cap_ = cap;
}

void Device::ensure_batch(size_t n) {
    if (n <= batch_cap_) return;
    size_t cap = batch_cap_ ? batch_cap_ : 1024;
    while (cap < n) cap *= 2;
    HIP_CHECK(hipStreamSynchronize(STREAM));
    (void)hipFree(d_ks_);
    if (lane_ == 0) {  // the gate staging ring belongs to lane 0 (lanes run resident plans only)
        (void)hipFree(d_gates_);
        for (auto& h : h_stage_) {
            if (h) (void)hipHostFree(h);
            h = nullptr;
        }
        HIP_CHECK(hipMalloc(&d_gates_, sizeof(DevGate) * cap));
        for (auto& h : h_stage_) HIP_CHECK(hipHostMalloc(&h, sizeof(DevGate) * cap));
    }
    HIP_CHECK(hipMalloc(&d_ks_, (size_t)8 * p_.ks_stride() * cap));
    batch_cap_ = cap;
}

int Device::alloc_slot() {
    if (!free_slots_.empty()) {
        int s = free_slots_.back();
        free_slots_.pop_back();
        return s;
    }
    ensure_arena(next_slot_ + 1);
    return (int)next_slot_++;
}
void Device::free_slot(int s) {
    if (s < 0) return;
    // a lane may still read or write it: recycled after the next host sync of every lane
    if (lanes_unsynced_ || lane_ != 0) {
        deferred_free_.push_back(s);
        // a serving loop that never downloads: recycle in bulk rather than grow the arena
        if (deferred_free_.size() >= (size_t)1 << 16) sync_all();
    } else {
        free_slots_.push_back(s);
    }
}

// packed copies between arena slots and a device buffer of the caller (the
// multi-rank exchange of a level's outputs: fr_shard_export / fr_shard_import):
// one workgroup per LWE, lwe_len u64 each, coalesced
__global__ void __launch_bounds__(256) k_slots_to_buf(const uint64_t* __restrict__ arena, int stride,
                                                      const int* __restrict__ slots, int len, uint64_t* __restrict__ buf) {
    const uint64_t* s = arena + (size_t)slots[blockIdx.x] * stride;
    uint64_t* d = buf + (size_t)blockIdx.x * len;
    for (int c = threadIdx.x; c < len; c += 256) d[c] = s[c];
}
__global__ void __launch_bounds__(256) k_buf_to_slots(const uint64_t* __restrict__ buf, int len,
                                                      const int* __restrict__ slots, int stride, uint64_t* __restrict__ arena) {
    const uint64_t* s = buf + (size_t)blockIdx.x * len;
    uint64_t* d = arena + (size_t)slots[blockIdx.x] * stride;
    for (int c = threadIdx.x; c < len; c += 256) d[c] = s[c];
}
struct SlotArgs {
    int s[16];
};
__global__ void __launch_bounds__(256) k_slots_to_buf_arg(const uint64_t* __restrict__ arena, int stride, SlotArgs sl,
                                                          int len, uint64_t* __restrict__ buf) {
    const uint64_t* s = arena + (size_t)sl.s[blockIdx.x] * stride;
    uint64_t* d = buf + (size_t)blockIdx.x * len;
    for (int c = threadIdx.x; c < len; c += 256) d[c] = s[c];
}
void Device::slots_to_device_async(const int* slots, size_t n, uint64_t* dst) {
    if (!n) return;
    if (n > 16) throw Error(FR_ERR_INVALID, "slots_to_device_async: at most 16 slots");
    SlotArgs a{};
    for (size_t i = 0; i < n; ++i) {
        if (slots[i] < 0 || (size_t)slots[i] >= next_slot_) throw Error(FR_ERR_INVALID, "slot list: slot out of range");
        a.s[i] = slots[i];
    }
    k_slots_to_buf_arg<<<(unsigned)n, 256, 0, STREAM>>>(d_arena_, p_.slot_stride(), a, p_.lwe_len(), dst);
    HIP_CHECK(hipGetLastError());
}
void Device::stage_slot_list(const int* slots, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (slots[i] < 0 || (size_t)slots[i] >= next_slot_) throw Error(FR_ERR_INVALID, "slot list: slot out of range");
    if (n > slot_list_cap_) {
        HIP_CHECK(hipStreamSynchronize(STREAM));
        (void)hipFree(d_slot_list_);
        d_slot_list_ = nullptr;
        slot_list_cap_ = std::max<size_t>(n, 1024);
        HIP_CHECK(hipMalloc(&d_slot_list_, 4 * slot_list_cap_));
    }
    HIP_CHECK(hipMemcpyAsync(d_slot_list_, slots, 4 * n, hipMemcpyHostToDevice, STREAM));
}
void Device::slots_to_device(const int* slots, size_t n, uint64_t* dst) {
    if (!n) return;
    stage_slot_list(slots, n);
    k_slots_to_buf<<<(unsigned)n, 256, 0, STREAM>>>(d_arena_, p_.slot_stride(), d_slot_list_, p_.lwe_len(), dst);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(STREAM));  // the caller's stream may read dst now
}
void Device::device_to_slots(const int* slots, size_t n, const uint64_t* src) {
    if (!n) return;
    stage_slot_list(slots, n);
    k_buf_to_slots<<<(unsigned)n, 256, 0, STREAM>>>(src, p_.lwe_len(), d_slot_list_, p_.slot_stride(), d_arena_);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(STREAM));  // the caller may reuse src now
}

void Device::write_slots(const int* slots, size_t n, const uint64_t* host) {
    const int L = p_.lwe_len(), S = p_.slot_stride();
    for (size_t i = 0; i < n; ++i)
        HIP_CHECK(hipMemcpyAsync(d_arena_ + (size_t)slots[i] * S, host + i * L, 8 * (size_t)L, hipMemcpyHostToDevice, STREAM));
    HIP_CHECK(hipStreamSynchronize(STREAM));
}
void Device::read_slot(int slot, uint64_t* host) {
    HIP_CHECK(hipMemcpyAsync(host, d_arena_ + (size_t)slot * p_.slot_stride(), 8 * (size_t)p_.lwe_len(),
                             hipMemcpyDeviceToHost, STREAM));
    sync_all();
}
void Device::zero_slot(int slot) {
    HIP_CHECK(hipMemsetAsync(d_arena_ + (size_t)slot * p_.slot_stride(), 0, 8 * (size_t)p_.lwe_len(), STREAM));
}

void Device::upload_keys(const std::vector<uint64_t>& ksk, const std::vector<uint64_t>& bsk) {
    if (ksk.size() != (size_t)p_.big() * p_.ks_level * (p_.n + 1)) throw Error(FR_ERR_INVALID, "ksk size");
    if (bsk.size() != p_.bsk_len()) throw Error(FR_ERR_INVALID, "bsk size");
    // every queued launch of every lane that reads the old keys has finished before they go
    HIP_CHECK(hipDeviceSynchronize());
    (void)hipFree(d_ksk_);
    (void)hipFree(d_bsk_);
    d_ksk_ = nullptr;
    d_bsk_ = nullptr;
    HIP_CHECK(hipMalloc(&d_ksk_, 8 * ksk.size()));
    HIP_CHECK(hipMemcpy(d_ksk_, ksk.data(), 8 * ksk.size(), hipMemcpyHostToDevice));
    (void)hipFree(d_tbsk_);  // host-generated keys: export reads the host copy
    d_tbsk_ = nullptr;
    build_ksk_limbs();
    if (p_.ring == FR_RING_FFT) upload_fft_bsk(bsk);
    else upload_rns_bsk(bsk);
}

bool Device::latency_shape(size_t n) const { return n <= (p_.ring == FR_RING_FFT ? fft_small_ : small_batch_); }
bool Device::pair_shape(size_t n) const { return p_.ring == FR_RING_FFT && !latency_shape(n) && n <= fft_pair_; }

void Device::launch_br(const DevGate* d_gates, const uint64_t* d_ks, size_t n, void* ev_start, void* ev_stop) {
    if (p_.ring == FR_RING_FFT) launch_br_fft(d_gates, d_ks, n, stream_, ev_start, ev_stop);
    else launch_br_rns(d_gates, d_ks, n, ev_start, ev_stop);
}

void Device::validate_gates(const DevGate* gates, size_t n, size_t n_refs) const {
    for (size_t i = 0; i < n; ++i) {
        const DevGate& g = gates[i];
        if (g.n_in < 0 || g.n_in > 16 || g.n_out < 1 || g.n_out > MAX_OUT || g.direct < 0 || g.direct > 2 ||
            (g.direct && g.n_out != 1))
            throw Error(FR_ERR_INVALID, "device gate: bad descriptor");
        for (int f = 0; f < g.n_out; ++f)
            if (g.out_slot[f] < 0 || (size_t)g.out_slot[f] >= next_slot_) throw Error(FR_ERR_INVALID, "device gate: bad output slot");
        for (int q = 0; q < g.n_in; ++q) {
            const int s = g.in_slot[q];
            if (s >= 0 ? (size_t)s >= next_slot_ : (size_t)(-1 - (int64_t)s) >= n_refs)
                throw Error(FR_ERR_INVALID, "device gate: bad input slot");
        }
    }
}

void Device::bind_content(const int* cmap, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (cmap[i] < -1 || (cmap[i] >= 0 && (size_t)cmap[i] >= next_slot_))
            throw Error(FR_ERR_INVALID, "content map: slot out of range");
    if (n > cmap_cap_) {
        HIP_CHECK(hipStreamSynchronize(STREAM));  // no launch may still read the old map
        (void)hipFree(d_cmap_);
        d_cmap_ = nullptr;
        for (auto& h : h_cmap_) {
            if (h) (void)hipHostFree(h);
            h = nullptr;
        }
        size_t cap = cmap_cap_ ? cmap_cap_ : 4096;
        while (cap < n) cap *= 2;
        HIP_CHECK(hipMalloc(&d_cmap_, 4 * cap));
        for (auto& h : h_cmap_) HIP_CHECK(hipHostMalloc(&h, 4 * cap));
        cmap_cap_ = cap;
    }
    // the map bound last is still in place (a replay of the same content): nothing to copy
    if (n == cmap_n_ && n && std::memcmp(h_cmap_[cmap_stage_], cmap, 4 * n) == 0) return;
    cmap_stage_ ^= 1;
    // the pinned buffer is rewritten only after its previous copy completed
    HIP_CHECK(hipEventSynchronize((hipEvent_t)cmap_ev_[cmap_stage_]));
    std::memcpy(h_cmap_[cmap_stage_], cmap, 4 * n);
    if (n) HIP_CHECK(hipMemcpyAsync(d_cmap_, h_cmap_[cmap_stage_], 4 * n, hipMemcpyHostToDevice, STREAM));
    HIP_CHECK(hipEventRecord((hipEvent_t)cmap_ev_[cmap_stage_], STREAM));
    cmap_n_ = n;
}

void Device::run_level(const DevGate* gates, size_t n) {
    if (!n) return;
    if (!has_keys()) throw Error(FR_ERR_NO_KEY, "server key not uploaded");
    if (lane_ != 0) throw Error(FR_ERR_INVALID, "staged gate batches run on lane 0 only");
    validate_gates(gates, n);
    ensure_batch(n);
    // d_gates_ / d_ks_ are reused in stream order (this level's copy runs after
    // the previous level's kernels); only the host staging buffer needs a wait
    std::memcpy(stage_acquire(), gates, sizeof(DevGate) * n);
    stage_copy(n);
    launch_level(d_gates_, gates, n);
}

void Device::run_level_resident(const DevGate* d_gates, const DevGate* host, size_t n, size_t n_refs) {
    if (!n) return;
    if (!has_keys()) throw Error(FR_ERR_NO_KEY, "server key not uploaded");
    if (n_refs > cmap_n_) throw Error(FR_ERR_INVALID, "template plan: content map not bound");
    ensure_batch(n);
    launch_level(d_gates, host, n);
}

DevGate* Device::upload_gates(const DevGate* gates, size_t n, size_t n_refs) {
    validate_gates(gates, n, n_refs);
    DevGate* d = nullptr;
    HIP_CHECK(hipMalloc(&d, sizeof(DevGate) * std::max<size_t>(n, 1)));
    HIP_CHECK(hipMemcpy(d, gates, sizeof(DevGate) * n, hipMemcpyHostToDevice));
    return d;
}

void Device::free_gates(DevGate* d) {
    if (!d) return;
    HIP_CHECK(hipStreamSynchronize(STREAM));
    HIP_CHECK(hipFree(d));
}

void Device::launch_level(const DevGate* d_gates, const DevGate* host, size_t n) {
    PendingTimer t{};
    if (profiling_)
        for (auto& e : t.ev) e = take_event();
    // keyswitch events at level 2 only: two more event-stamped launches per level cost
    // ~30 us per /abc/ match (tools/match_probe.py).  Level 1 stamps stop events only: the
    // blind rotation runs from the keyswitch's end event to its own (the launch gap between
    // them, ~0 without a start event, counts as rotation time).  A start event on the BR
    // launch opened a ~6.6 us gap before it and the stop events ~4.7 us after it under the
    // kernel trace (profiles/r04/gaps/).
    t.chain = profiling_ == 1 && timer_chain_;
    if (profiling_ >= 2) launch_ks(d_gates, n, d_ks_, t.ev[0], t.ev[1]);
    else launch_ks(d_gates, n, d_ks_, nullptr, t.chain ? t.ev[1] : nullptr);
    launch_br(d_gates, d_ks_, n, t.chain ? nullptr : t.ev[2], t.ev[3]);
    HIP_CHECK(hipGetLastError());
    if (profiling_) {
        t.gates = n;
        t.lat = latency_shape(n);
        t.pair = pair_shape(n) && !fft_dual_;  // FR_FFT_DUAL launches: one bootstrap per workgroup
        t.ks = profiling_ >= 2;
        t.outs = 0;
        for (size_t i = 0; i < n; ++i) t.outs += host[i].n_out;
        pending_.push_back(t);
    }
}

DevGate* Device::stage_acquire() {
    stage_ ^= 1;
    HIP_CHECK(hipEventSynchronize((hipEvent_t)stage_ev_[stage_]));  // never-recorded events are complete
    return h_stage_[stage_];
}
void Device::stage_copy(size_t n) {
    HIP_CHECK(hipMemcpyAsync(d_gates_, h_stage_[stage_], sizeof(DevGate) * n, hipMemcpyHostToDevice, STREAM));
    HIP_CHECK(hipEventRecord((hipEvent_t)stage_ev_[stage_], STREAM));
}
void* Device::take_event() {
    if (!event_pool_.empty()) {
        void* e = event_pool_.back();
        event_pool_.pop_back();
        return e;
    }
    // timing-only events (read after a stream sync): a device-scope release instead of
    // the system-scope fence, so recording one between two launches costs no cache
    // writeback (with the default fence each record opened a ~5 us gap in the level chain)
    // (the first flag set this runtime accepts)
    hipEvent_t ev = nullptr;
    for (unsigned fl : {(unsigned)hipEventReleaseToDevice, (unsigned)hipEventDisableSystemFence, (unsigned)hipEventDefault})
        if (hipEventCreateWithFlags(&ev, fl) == hipSuccess) return ev;
        else (void)hipGetLastError();
    HIP_CHECK(hipEventCreate(&ev));
    return ev;
}
// KS / BR kernel times of the levels issued since the last sync (HIP events
// on the launch stream, read once the stream has drained)
void Device::resolve_timers() {
    for (auto& t : pending_) {
        float ks = 0, br = 0;
        if (t.ks) HIP_CHECK(hipEventElapsedTime(&ks, (hipEvent_t)t.ev[0], (hipEvent_t)t.ev[1]));
        HIP_CHECK(hipEventElapsedTime(&br, (hipEvent_t)t.ev[t.chain ? 1 : 2], (hipEvent_t)t.ev[3]));
        timers_.ks_ms += ks;
        timers_.br_ms += br;
        timers_.br_launches += 1;
        timers_.br_gates += t.gates;
        timers_.lut_outputs += t.outs;
        if (t.lat) {
            timers_.lat_br_ms += br;
            timers_.lat_launches += 1;
            timers_.lat_gates += t.gates;
        }
        if (t.pair) {
            timers_.pair_br_ms += br;
            timers_.pair_launches += 1;
            timers_.pair_gates += t.gates;
        }
        for (auto* e : t.ev) event_pool_.push_back(e);
    }
    pending_.clear();
}

void Device::sync() {
    sync_all();
    resolve_timers();
}

// ---------------------------------------------------------------- tests
void Device::keyswitch_host(const uint64_t* in, size_t count, uint64_t* out) {
    if (!has_keys()) throw Error(FR_ERR_NO_KEY, "server key not uploaded");
    HIP_CHECK(hipStreamSynchronize(STREAM));  // queued matches read d_ks_ / d_gates_ (blind_rotate_host)
    std::vector<int> slots(count);
    std::vector<DevGate> gates(count);
    for (size_t i = 0; i < count; ++i) slots[i] = alloc_slot();
    write_slots(slots.data(), count, in);
    for (size_t i = 0; i < count; ++i) {
        std::memset(&gates[i], 0, sizeof(DevGate));
        gates[i].n_in = 1;
        gates[i].in_slot[0] = slots[i];
        gates[i].in_w[0] = 1;
        gates[i].n_out = 1;
        gates[i].direct = JOB_DIRECT;
        gates[i].out_slot[0] = slots[i];
    }
    ensure_batch(count);
    HIP_CHECK(hipMemcpy(d_gates_, gates.data(), sizeof(DevGate) * count, hipMemcpyHostToDevice));
    launch_ks(d_gates_, count, d_ks_);
    HIP_CHECK(hipStreamSynchronize(STREAM));
    const int ks = p_.ks_stride();
    for (size_t i = 0; i < count; ++i)
        HIP_CHECK(hipMemcpy(out + i * (p_.n + 1), d_ks_ + i * ks, 8 * (size_t)(p_.n + 1), hipMemcpyDeviceToHost));
    for (int s : slots) free_slot(s);
}

// a blind-rotation job without inputs: n_out LUTs of 16 bytes, output slots filled in by run_br_jobs
static DevGate br_job(const uint8_t* luts, int n_out, int direct) {
    DevGate g;
    std::memset(&g, 0, sizeof g);
    g.n_out = n_out;
    g.direct = direct;
    std::memcpy(g.lut, luts, 16 * (size_t)n_out);
    return g;
}

// one launch of `gates` on the keyswitched inputs ks_in (n + 1 words each); the outputs of
// gate i follow those of gate i - 1 in out (lwe_len words each)
void Device::run_br_jobs(const uint64_t* ks_in, std::vector<DevGate>& gates, uint64_t* out) {
    if (!has_keys()) throw Error(FR_ERR_NO_KEY, "server key not uploaded");
    // an asynchronous match may still read d_ks_ / d_gates_ on STREAM; the plain
    // copies below run on the null stream, which does not wait for a non-blocking one
    HIP_CHECK(hipStreamSynchronize(STREAM));
    const size_t count = gates.size();
    ensure_batch(count);
    const int ks = p_.ks_stride();
    for (size_t i = 0; i < count; ++i)
        HIP_CHECK(hipMemcpy(d_ks_ + i * ks, ks_in + i * (p_.n + 1), 8 * (size_t)(p_.n + 1), hipMemcpyHostToDevice));
    std::vector<int> slots;
    for (auto& g : gates)
        for (int f = 0; f < g.n_out; ++f) {
            slots.push_back(alloc_slot());
            g.out_slot[f] = slots.back();
        }
    HIP_CHECK(hipMemcpy(d_gates_, gates.data(), sizeof(DevGate) * count, hipMemcpyHostToDevice));
    launch_br(d_gates_, d_ks_, count);
    HIP_CHECK(hipStreamSynchronize(STREAM));
    for (size_t i = 0; i < slots.size(); ++i) read_slot(slots[i], out + i * p_.lwe_len());
    for (int s : slots) free_slot(s);
}

void Device::blind_rotate_host(const uint64_t* ks_in, const uint8_t* luts, size_t count, uint64_t* out) {
    std::vector<DevGate> gates(count);
    for (size_t i = 0; i < count; ++i) gates[i] = br_job(luts + 16 * i, 1, JOB_DIRECT);
    run_br_jobs(ks_in, gates, out);
}

void Device::blind_rotate_multi_host(const uint64_t* ks_in, const uint8_t* luts, int n_out, int direct,
                                     uint64_t* out) {
    if (!has_keys()) throw Error(FR_ERR_NO_KEY, "server key not uploaded");
    if (n_out < 1 || n_out > MAX_OUT || direct < 0 || direct > 2 || (direct && n_out != 1))
        throw Error(FR_ERR_INVALID, "bad n_out");
    std::vector<DevGate> gates{br_job(luts, n_out, direct)};
    run_br_jobs(ks_in, gates, out);
}

int lut_w_norm2(const uint8_t* lut) {
    int s = 0;
    for (int m = 1; m < 16; ++m) s += ((int)lut[m] - lut[m - 1]) * ((int)lut[m] - lut[m - 1]);
    s += ((int)lut[0] + lut[15]) * ((int)lut[0] + lut[15]);
    return s;
}

void Device::bench_pbs(const std::vector<DevGate>& gates, int iters, double* br_ms, double* total_ms) {
    const size_t n = gates.size();
    ensure_batch(n);
    sync();
    std::memcpy(stage_acquire(), gates.data(), sizeof(DevGate) * n);
    stage_copy(n);
    float br_sum = 0;
    HIP_CHECK(hipEventRecord((hipEvent_t)ev_[3], STREAM));
    for (int it = 0; it < iters; ++it) {
        launch_ks(d_gates_, n, d_ks_);
        HIP_CHECK(hipEventRecord((hipEvent_t)ev_[1], STREAM));
        launch_br(d_gates_, d_ks_, n);
        HIP_CHECK(hipEventRecord((hipEvent_t)ev_[2], STREAM));
        HIP_CHECK(hipEventSynchronize((hipEvent_t)ev_[2]));
        float br = 0;
        HIP_CHECK(hipEventElapsedTime(&br, (hipEvent_t)ev_[1], (hipEvent_t)ev_[2]));
        br_sum += br;
    }
    HIP_CHECK(hipEventRecord((hipEvent_t)ev_[0], STREAM));
    HIP_CHECK(hipEventSynchronize((hipEvent_t)ev_[0]));
    float tot = 0;
    HIP_CHECK(hipEventElapsedTime(&tot, (hipEvent_t)ev_[3], (hipEvent_t)ev_[0]));
    *br_ms = br_sum;
    *total_ms = tot;
}

}  // namespace fr
