// The Device host class (HIP, gfx950): the HIP side of the resource owners (owned.h) and the
// staging ring, context construction, streams and lanes, the arena
// of big-LWE slots and its packed slot copies, gate staging and validation, running a
// dependency level (keyswitch + blind rotation), timers, and the single-stage entry points
// of the parity tests.  The kernels of a level live with the methods that launch them:
// rns_br.hip (RNS blind rotation), fft_br.hip (FFT blind rotation), keyswitch.hip,
// keygen.hip (server-key generation, encryption), and select_sum.hip (the extract-sums of a
// find over clear content, which run before a plan's first level).
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

// ---------------------------------------------------------------- owners (owned.h)
namespace gpu {
void* dev_alloc(size_t bytes) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, bytes));
    return p;
}
void dev_free(void* p) noexcept { (void)hipFree(p); }
void* pinned_alloc(size_t bytes) {
    void* p = nullptr;
    HIP_CHECK(hipHostMalloc(&p, bytes));
    return p;
}
void pinned_free(void* p) noexcept { (void)hipHostFree(p); }
hipEvent_t event_create(unsigned flags) {
    hipEvent_t e = nullptr;
    HIP_CHECK(hipEventCreateWithFlags(&e, flags));
    return e;
}
void event_destroy(hipEvent_t e) noexcept { (void)hipEventDestroy(e); }
hipStream_t stream_create() {
    hipStream_t s = nullptr;
    HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return s;
}
void stream_destroy(hipStream_t s) noexcept { (void)hipStreamDestroy(s); }

void StagingBytes::reserve(size_t bytes, size_t first, hipStream_t s) {
    if (bytes <= d_.size()) return;
    size_t cap = d_.size() ? d_.size() : first;
    while (cap < bytes) cap *= 2;
    HIP_CHECK(hipStreamSynchronize(s));  // no copy or kernel may still use the old buffers
    d_.reset();
    for (auto& h : h_) h.reset();
    try {
        for (auto& e : ev_)
            if (!e) e = Event(hipEventDisableTiming);
        for (auto& h : h_) h.alloc(cap);
        d_.alloc(cap);
    } catch (...) {
        for (auto& h : h_) h.reset();
        throw;
    }
}
void* StagingBytes::acquire() {
    side_ ^= 1;
    HIP_CHECK(hipEventSynchronize(ev_[side_].get()));
    return h_[side_].get();
}
void StagingBytes::commit(size_t bytes, hipStream_t s) {
    HIP_CHECK(hipMemcpyAsync(d_.get(), h_[side_].get(), bytes, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(ev_[side_].get(), s));
}
}  // namespace gpu

Device::Device(const Params& p, int device) : p_(p), dev_(device) {
    if (!supported(p)) throw Error(FR_ERR_INVALID, "device: unsupported (k, N)");
    if (p.ks_base_log != 3 || p.ks_level != 5 || p.pbs_base_log != 23 || p.pbs_level != 1)
        throw Error(FR_ERR_INVALID, "device: only KS 2^3x5 and PBS 2^23x1 are compiled");
    if (p.n > 1024) throw Error(FR_ERR_INVALID, "device: n > 1024");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= device || device < 0)
        throw Error(FR_ERR_NO_DEVICE, "no usable HIP device " + std::to_string(device));
    HIP_CHECK(hipSetDevice(device));
    lane0_.stream.create();
    for (auto& e : ev_) e = gpu::Event(hipEventDefault);
    init_rns();  // (an FFT-ring context too: twiddles and kernel attributes)
    init_ks();
    if (const char* ev = std::getenv("FR_TIMER_CHAIN")) timer_chain_ = std::atoi(ev) != 0;
    if (p.ring == FR_RING_FFT) init_fft();
    ensure_arena(1024);
    ensure_ks(1024);
    ensure_gates(1024);
}

// Nothing may be released while a launch could still use it, and a stream not before the work
// on it ended: wait for every lane, then the members go (device.h: the lanes last).
Device::~Device() {
    (void)hipSetDevice(dev_);
    for (auto& l : lanes_) (void)hipStreamSynchronize(l.stream.get());
    if (lane0_.stream) (void)hipStreamSynchronize(lane0_.stream.get());
}

// ---------------------------------------------------------------- lanes
void Device::set_lanes(int n) {
    if (n < 1 || n > 8) throw Error(FR_ERR_INVALID, "lanes: 1..8");
    if (lane_ != 0) throw Error(FR_ERR_INVALID, "lanes: changed inside a lane");
    sync_all();
    // n >= 2: n lanes besides lane 0 (matches go to them only: a match on lane 0 would wait
    // for the other lanes at its first launch)
    const int extra = n >= 2 ? n : 0;
    while ((int)lanes_.size() > extra) lanes_.pop_back();
    if (!main_ev_ && extra) main_ev_ = gpu::Event(hipEventDisableTiming);
    while ((int)lanes_.size() < extra) {
        LaneState l;
        l.stream.create();
        l.done_ev = gpu::Event(hipEventDisableTiming);
        lanes_.push_back(std::move(l));
        // the lane's keyswitch scratch at the main lane's size (ensure_ks on entry grows it)
        enter_lane((int)lanes_.size());
        ensure_ks(1024);
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
    HIP_CHECK(hipEventRecord(main_ev_.get(), lane0_.stream.get()));
    HIP_CHECK(hipStreamWaitEvent(lanes_[i - 1].stream.get(), main_ev_.get(), 0));
    lane_ = i;
}
void Device::leave_lane() {
    if (lane_ == 0) return;
    LaneState& l = cur();
    HIP_CHECK(hipEventRecord(l.done_ev.get(), l.stream.get()));
    l.pending = true;
    lanes_pending_ = true;
    lanes_unsynced_ = true;
    lane_ = 0;
}
void Device::join_lanes() {
    if (!lanes_pending_ || lane_ != 0) return;
    for (auto& l : lanes_)
        if (l.pending) {
            HIP_CHECK(hipStreamWaitEvent(lane0_.stream.get(), l.done_ev.get(), 0));
            l.pending = false;
        }
    lanes_pending_ = false;
}
hipStream_t Device::cur_stream() {
    if (lane_ == 0 && lanes_pending_) join_lanes();
    return cur().stream.get();
}
void Device::sync_all() {
    HIP_CHECK(hipStreamSynchronize(lane0_.stream.get()));
    for (auto& l : lanes_) HIP_CHECK(hipStreamSynchronize(l.stream.get()));
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
    const size_t stride = p_.slot_stride(), have = d_arena_.size() / stride;
    if (slots <= have) return;
    size_t cap = have ? have : 1024;
    while (cap < slots) cap *= 2;
    gpu::DevBuf<uint64_t> nb(stride * cap);
    if (d_arena_) {
        sync_all();  // no launch of any lane may still use the old arena
        HIP_CHECK(hipMemcpyAsync(nb.get(), d_arena_.get(), 8 * d_arena_.size(), hipMemcpyDeviceToDevice, STREAM));
        HIP_CHECK(hipStreamSynchronize(STREAM));
    }
    d_arena_ = std::move(nb);
}

void Device::ensure_ks(size_t n) {
    const size_t row = p_.ks_stride();
    if (n * row <= cur().ks.size()) return;
    HIP_CHECK(hipStreamSynchronize(STREAM));
    cur().ks.grow(n * row, 1024 * row);
}
void Device::ensure_gates(size_t n) { gates_.reserve(n, 1024, STREAM); }

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
    k_slots_to_buf_arg<<<(unsigned)n, 256, 0, STREAM>>>(d_arena_.get(), p_.slot_stride(), a, p_.lwe_len(), dst);
    HIP_CHECK(hipGetLastError());
}
void Device::stage_slot_list(const int* slots, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (slots[i] < 0 || (size_t)slots[i] >= next_slot_) throw Error(FR_ERR_INVALID, "slot list: slot out of range");
    if (n > d_slot_list_.size()) {
        HIP_CHECK(hipStreamSynchronize(STREAM));
        d_slot_list_.alloc(std::max<size_t>(n, 1024));
    }
    HIP_CHECK(hipMemcpyAsync(d_slot_list_.get(), slots, 4 * n, hipMemcpyHostToDevice, STREAM));
}
void Device::slots_to_device(const int* slots, size_t n, uint64_t* dst) {
    if (!n) return;
    stage_slot_list(slots, n);
    k_slots_to_buf<<<(unsigned)n, 256, 0, STREAM>>>(d_arena_.get(), p_.slot_stride(), d_slot_list_.get(), p_.lwe_len(), dst);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(STREAM));  // the caller's stream may read dst now
}
void Device::device_to_slots(const int* slots, size_t n, const uint64_t* src) {
    if (!n) return;
    stage_slot_list(slots, n);
    k_buf_to_slots<<<(unsigned)n, 256, 0, STREAM>>>(src, p_.lwe_len(), d_slot_list_.get(), p_.slot_stride(), d_arena_.get());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(STREAM));  // the caller may reuse src now
}

void Device::write_slots(const int* slots, size_t n, const uint64_t* host) {
    const int L = p_.lwe_len(), S = p_.slot_stride();
    for (size_t i = 0; i < n; ++i)
        HIP_CHECK(hipMemcpyAsync(d_arena_.get() + (size_t)slots[i] * S, host + i * L, 8 * (size_t)L, hipMemcpyHostToDevice, STREAM));
    HIP_CHECK(hipStreamSynchronize(STREAM));
}
void Device::read_slot(int slot, uint64_t* host) {
    HIP_CHECK(hipMemcpyAsync(host, d_arena_.get() + (size_t)slot * p_.slot_stride(), 8 * (size_t)p_.lwe_len(),
                             hipMemcpyDeviceToHost, STREAM));
    sync_all();
}
void Device::zero_slot(int slot) {
    HIP_CHECK(hipMemsetAsync(d_arena_.get() + (size_t)slot * p_.slot_stride(), 0, 8 * (size_t)p_.lwe_len(), STREAM));
}

void Device::upload_keys(const std::vector<uint64_t>& ksk, const std::vector<uint64_t>& bsk) {
    if (ksk.size() != (size_t)p_.big() * p_.ks_level * (p_.n + 1)) throw Error(FR_ERR_INVALID, "ksk size");
    if (bsk.size() != p_.bsk_len()) throw Error(FR_ERR_INVALID, "bsk size");
    Replacing key_guard([this] { drop_server_key(); });  // (no torus BSK here: export reads the host copy)
    ksk_.alloc_rows(p_.big() * p_.ks_level, p_.n + 1);
    HIP_CHECK(hipMemcpy(ksk_.rows.get(), ksk.data(), 8 * ksk.size(), hipMemcpyHostToDevice));
    build_limbs(ksk_);
    if (p_.ring == FR_RING_FFT) upload_fft_bsk(bsk);
    else upload_rns_bsk(bsk);
    key_guard.dismiss();
}

// The one place that decides a launch's shape: launch_br_fft and launch_br_rns switch on it and
// the timers read it.  Small launches (at most one bootstrap per CU): the latency shape, the
// smallest (FFT ring, k = 1, at most fft_kpre_) with their key products formed first.  Selector
// launches take the shape by count alone: never the key products, never the dual.
BrShape Device::br_shape(size_t n, bool acc) const {
    if (p_.ring != FR_RING_FFT) return n <= small_batch_ ? BrShape::Latency : BrShape::Throughput;
    if (n <= fft_small_) return n <= fft_kpre_ && p_.k == 1 && !acc ? BrShape::LatencyKP : BrShape::Latency;
    if (n <= fft_pair_ && p_.k == 1) return fft_dual_ && !acc ? BrShape::Dual : BrShape::Pair;
    return BrShape::Throughput;
}
void Device::PendingTimer::count_as(BrShape shape) {
    lat = shape == BrShape::Latency || shape == BrShape::LatencyKP;
    pair = shape == BrShape::Pair;  // (the dual: one bootstrap per workgroup)
}

void Device::launch_br(const DevGate* d_gates, const uint64_t* d_ks, size_t n, hipEvent_t ev_start, hipEvent_t ev_stop,
                       bool acc) {
    if (acc && p_.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "private search: FFT ring only");
    if (p_.ring == FR_RING_FFT) launch_br_fft(d_gates, d_ks, n, cur().stream.get(), ev_start, ev_stop, acc);
    else launch_br_rns(d_gates, d_ks, n, ev_start, ev_stop);
}

void Device::validate_gates(const DevGate* gates, size_t n, size_t n_refs) const {
    for (size_t i = 0; i < n; ++i) {
        const DevGate& g = gates[i];
        if (g.n_in < 0 || g.n_in > 16 || g.n_out < 1 || g.n_out > MAX_OUT || g.direct < 0 || g.direct > JOB_ACC ||
            (g.direct && g.n_out != 1))
            throw Error(FR_ERR_INVALID, "device gate: bad descriptor");
        if (g.direct == JOB_ACC) {
            if (p_.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "private search: FFT ring only");
            if (acc_selector(g) >= (uint32_t)MAX_SELECTORS) throw Error(FR_ERR_INVALID, "device gate: bad selector index");
        }
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
    LaneState& l = cur();
    const size_t bound = l.cmap_n;
    l.cmap_n = 0;  // (an error below leaves no map bound)
    if (!n) return;
    const hipStream_t s = STREAM;
    l.cmap.reserve(n, 4096, s);  // (after a reallocation no launch reads the old map)
    // the map bound last is still in place (a replay of the same content): nothing to copy
    if (n != bound || std::memcmp(l.cmap.last(), cmap, 4 * n) != 0) {
        std::memcpy(l.cmap.acquire(), cmap, 4 * n);
        l.cmap.commit(n, s);
    }
    l.cmap_n = n;
}

DevNeedle::~DevNeedle() {
    if (!words || !dev) return;
    try {
        dev->sync();
    } catch (...) {  // (the buffer goes all the same)
    }
}

DevNeedle Device::upload_needle(const uint64_t* words, size_t m, NeedleForm form) {
    if (p_.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "private search: FFT ring only");
    if (!words || m < 1 || 2 * m > (size_t)MAX_SELECTORS) throw Error(FR_ERR_INVALID, "needle: 1 <= m <= 64");
    DevNeedle nd;
    nd.dev = this;
    nd.m = m;
    nd.form = form;
    const size_t tpg = (size_t)p_.N / 256;  // byte tables per selector
    if (form == NEEDLE_BYTES && !tpg) throw Error(FR_ERR_INVALID, "byte needle: N is not a multiple of 256");
    nd.words.alloc((form == NEEDLE_BYTES ? (m + tpg - 1) / tpg : 2 * m) * (size_t)(p_.k + 1) * p_.N);
    HIP_CHECK(hipMemcpy(nd.words.get(), words, 8 * nd.words.size(), hipMemcpyHostToDevice));
    return nd;
}

void Device::bind_selectors(const uint64_t* table, size_t count, NeedleForm form) {
    if (table && p_.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "private search: FFT ring only");
    cur().sel = table;
    cur().sel_n = table ? count : 0;
    cur().sel_form = table ? form : NEEDLE_NIBBLES;
}

size_t Device::leading_selector_jobs(const DevGate* host, size_t n) const {
    // build_schedule puts a level's selector jobs first: a batch that does not begin with one
    // has none, and every match without a needle leaves here
    if (!n || host[0].direct != JOB_ACC) return 0;
    size_t a = 0;
    while (a < n && host[a].direct == JOB_ACC) ++a;
    for (size_t i = 0; i < n; ++i) {
        if (host[i].direct != JOB_ACC) continue;
        if (i >= a) throw Error(FR_ERR_INVALID, "selector jobs must lead their level");
        if (cur().sel_form != NEEDLE_NIBBLES)
            throw Error(FR_ERR_INVALID, "selector job: a byte-table needle is read by extract-sums only");
        if ((size_t)acc_selector(host[i]) >= cur().sel_n)
            throw Error(FR_ERR_INVALID, "selector job: index past the selector table bound");
    }
    return a;
}

void Device::run_level(const DevGate* gates, size_t n) {
    if (!n) return;
    if (!has_keys()) throw Error(FR_ERR_NO_KEY, "server key not uploaded");
    if (lane_ != 0) throw Error(FR_ERR_INVALID, "staged gate batches run on lane 0 only");
    validate_gates(gates, n);
    ensure_ks(n);
    ensure_gates(n);
    // the device copy and the keyswitch scratch are reused in stream order (this level's
    // copy runs after the previous level's kernels); only the host staging buffer needs a wait
    std::memcpy(gates_.acquire(), gates, sizeof(DevGate) * n);
    gates_.commit(n, STREAM);
    launch_level(gates_.device(), gates, n);
}

void Device::run_level_resident(const DevGate* d_gates, const DevGate* host, size_t n, size_t n_refs) {
    if (!n) return;
    if (!has_keys()) throw Error(FR_ERR_NO_KEY, "server key not uploaded");
    if (n_refs > cur().cmap_n) throw Error(FR_ERR_INVALID, "template plan: content map not bound");
    ensure_ks(n);
    launch_level(d_gates, host, n);
}

gpu::DevBuf<DevGate> Device::upload_gates(const DevGate* gates, size_t n, size_t n_refs) {
    validate_gates(gates, n, n_refs);
    gpu::DevBuf<DevGate> d(std::max<size_t>(n, 1));
    HIP_CHECK(hipMemcpy(d.get(), gates, sizeof(DevGate) * n, hipMemcpyHostToDevice));
    return d;
}

// a level's selector jobs (they lead it) are launched apart from its other jobs
void Device::launch_level(const DevGate* d_gates, const DevGate* host, size_t n) {
    const size_t a = leading_selector_jobs(host, n);
    if (a) launch_jobs(d_gates, host, a, true);
    if (n > a) launch_jobs(d_gates + a, host + a, n - a, false);
}

void Device::launch_jobs(const DevGate* d_gates, const DevGate* host, size_t n, bool acc) {
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
    uint64_t* d_ks = cur().ks.get();
    if (profiling_ >= 2) launch_ks(d_gates, n, d_ks, t.ev[0].get(), t.ev[1].get());
    else launch_ks(d_gates, n, d_ks, nullptr, t.chain ? t.ev[1].get() : nullptr);
    launch_br(d_gates, d_ks, n, t.chain ? nullptr : t.ev[2].get(), t.ev[3].get(), acc);
    HIP_CHECK(hipGetLastError());
    if (profiling_) {
        t.gates = n;
        t.count_as(br_shape(n, acc));
        t.ks = profiling_ >= 2;
        t.outs = 0;
        for (size_t i = 0; i < n; ++i) t.outs += host[i].n_out;
        pending_.push_back(std::move(t));
    }
}

gpu::Event Device::take_event() {
    if (!event_pool_.empty()) {
        gpu::Event e = std::move(event_pool_.back());
        event_pool_.pop_back();
        return e;
    }
    // timing-only events (read after a stream sync): a device-scope release instead of
    // the system-scope fence, so recording one between two launches costs no cache
    // writeback (with the default fence each record opened a ~5 us gap in the level chain)
    // (the first flag set this runtime accepts)
    for (unsigned fl : {(unsigned)hipEventReleaseToDevice, (unsigned)hipEventDisableSystemFence})
        try {
            return gpu::Event(fl);
        } catch (const Error&) {
            (void)hipGetLastError();
        }
    return gpu::Event(hipEventDefault);
}
// KS / BR kernel times of the levels issued since the last sync (HIP events
// on the launch stream, read once the stream has drained)
void Device::resolve_timers() {
    for (auto& t : pending_) {
        float ks = 0, br = 0;
        if (t.ks) HIP_CHECK(hipEventElapsedTime(&ks, t.ev[0].get(), t.ev[1].get()));
        HIP_CHECK(hipEventElapsedTime(&br, t.ev[t.chain ? 1 : 2].get(), t.ev[3].get()));
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
        for (auto& e : t.ev)  // (a timer that stamped fewer than four holds empty ones)
            if (e) event_pool_.push_back(std::move(e));
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
    HIP_CHECK(hipStreamSynchronize(STREAM));  // queued matches read the scratch and the gate ring (blind_rotate_host)
    Slots slots(*this, count);
    std::vector<DevGate> gates(count);
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
    ensure_ks(count);
    ensure_gates(count);
    uint64_t* d_ks = cur().ks.get();
    HIP_CHECK(hipMemcpy(gates_.device(), gates.data(), sizeof(DevGate) * count, hipMemcpyHostToDevice));
    launch_ks(gates_.device(), count, d_ks);
    HIP_CHECK(hipStreamSynchronize(STREAM));
    const int ks = p_.ks_stride();
    for (size_t i = 0; i < count; ++i)
        HIP_CHECK(hipMemcpy(out + i * (p_.n + 1), d_ks + i * ks, 8 * (size_t)(p_.n + 1), hipMemcpyDeviceToHost));
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
    // an asynchronous match may still read the scratch and the gate ring on STREAM; the plain
    // copies below run on the null stream, which does not wait for a non-blocking one
    HIP_CHECK(hipStreamSynchronize(STREAM));
    const size_t count = gates.size();
    ensure_ks(count);
    ensure_gates(count);
    uint64_t* d_ks = cur().ks.get();
    const int ks = p_.ks_stride();
    for (size_t i = 0; i < count; ++i)
        HIP_CHECK(hipMemcpy(d_ks + i * ks, ks_in + i * (p_.n + 1), 8 * (size_t)(p_.n + 1), hipMemcpyHostToDevice));
    size_t n_out = 0;
    for (auto& g : gates) n_out += (size_t)g.n_out;
    Slots slots(*this, n_out);
    n_out = 0;
    for (auto& g : gates)
        for (int f = 0; f < g.n_out; ++f) g.out_slot[f] = slots[n_out++];
    HIP_CHECK(hipMemcpy(gates_.device(), gates.data(), sizeof(DevGate) * count, hipMemcpyHostToDevice));
    const size_t a = leading_selector_jobs(gates.data(), count);
    if (a && a != count) throw Error(FR_ERR_INVALID, "a launch is all selector jobs or none");
    // under fr_set_profiling the launch is stamped by its own dispatch, as a level's is, and
    // counts in the timers (tools/needle_probe.py compares the two kinds of launch by them)
    PendingTimer t{};
    if (profiling_) {
        t.ev[2] = take_event(), t.ev[3] = take_event();
        t.gates = count, t.outs = n_out;
        t.count_as(br_shape(count, a != 0));
    }
    launch_br(gates_.device(), d_ks, count, t.ev[2].get(), t.ev[3].get(), a != 0);
    if (profiling_) {
        pending_.push_back(std::move(t));
        sync();  // every lane: the pending timers of queued matches are resolved with this one
    } else {
        HIP_CHECK(hipStreamSynchronize(STREAM));
    }
    for (size_t i = 0; i < slots.size(); ++i) read_slot(slots[i], out + i * p_.lwe_len());
}

void Device::blind_rotate_acc_host(const uint64_t* ks_in, const uint64_t* accs, size_t count, uint64_t* out) {
    if (p_.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "private search: FFT ring only");
    if (!has_keys()) throw Error(FR_ERR_NO_KEY, "server key not uploaded");
    if (lane_ != 0) throw Error(FR_ERR_INVALID, "parity hooks run on lane 0 only");
    if (!count) return;
    // each job its own accumulator: the table of this call alone, indices past MAX_SELECTORS allowed
    const size_t W = (size_t)(p_.k + 1) * p_.N;
    gpu::DevBuf<uint64_t> table(count * W);
    HIP_CHECK(hipMemcpy(table.get(), accs, 8 * count * W, hipMemcpyHostToDevice));
    std::vector<DevGate> gates(count);
    for (size_t i = 0; i < count; ++i) {
        std::memset(&gates[i], 0, sizeof(DevGate));
        gates[i].n_out = 1;
        gates[i].direct = JOB_ACC;
        set_acc_selector(gates[i], (uint32_t)i);
    }
    const uint64_t* prev = cur().sel;
    const size_t prev_n = cur().sel_n;
    const NeedleForm prev_form = cur().sel_form;
    bind_selectors(table.get(), count);
    try {
        run_br_jobs(ks_in, gates, out);  // (synchronises before it returns: the table may go)
    } catch (...) {
        (void)hipStreamSynchronize(cur().stream.get());
        bind_selectors(prev, prev_n, prev_form);
        throw;
    }
    bind_selectors(prev, prev_n, prev_form);
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
    ensure_ks(n);
    ensure_gates(n);
    sync();
    std::memcpy(gates_.acquire(), gates.data(), sizeof(DevGate) * n);
    gates_.commit(n, STREAM);
    const DevGate* d_gates = gates_.device();
    uint64_t* d_ks = cur().ks.get();
    float br_sum = 0;
    HIP_CHECK(hipEventRecord(ev_[3].get(), STREAM));
    for (int it = 0; it < iters; ++it) {
        launch_ks(d_gates, n, d_ks);
        HIP_CHECK(hipEventRecord(ev_[1].get(), STREAM));
        launch_br(d_gates, d_ks, n);
        HIP_CHECK(hipEventRecord(ev_[2].get(), STREAM));
        HIP_CHECK(hipEventSynchronize(ev_[2].get()));
        float br = 0;
        HIP_CHECK(hipEventElapsedTime(&br, ev_[1].get(), ev_[2].get()));
        br_sum += br;
    }
    HIP_CHECK(hipEventRecord(ev_[0].get(), STREAM));
    HIP_CHECK(hipEventSynchronize(ev_[0].get()));
    float tot = 0;
    HIP_CHECK(hipEventElapsedTime(&tot, ev_[3].get(), ev_[0].get()));
    *br_ms = br_sum;
    *total_ms = tot;
}

}  // namespace fr
