// Device executor interface (HIP, gfx950), free of HIP headers: the engine compiles it with
// g++.  The host class is in device.hip; the kernels and the methods that launch them in
// rns_br.hip, fft_br.hip, keyswitch.hip and keygen.hip.  Every GPU resource of the class is
// held by an owner from owned.h, so ~Device only synchronises and the members release
// themselves in reverse order of declaration.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "common.h"
#include "owned.h"

namespace fr {

constexpr int MAX_OUT = 8;
// One blind-rotation job as the device sees it:
//   c = offset*2^58 + sum_q w_q * arena[in_slot_q];  KS; blind rotation of the
//   test polynomial; out_slot[f] <- LUT_f(c) for f < n_out.
// direct = 1: the test polynomial is LUT_0's own (one output).  direct = 0:
// multi-value bootstrapping, test polynomial (Delta/2)*sum_j X^j and one
// sparse small-integer product w_f per output (see k_blind_rotate).
// direct = 2: sign gate, test polynomial (Delta/2)*sum_j X^j, one output
// [c > 0] obtained as +-Delta/2 + Delta/2.
// direct = 3: selector job (private search), one output.  The rotation starts from a GLWE
// ciphertext of a direct test polynomial, selector acc_selector(gate) of the table bound last
// (bind_selectors), instead of from a LUT's own; sample extract as direct = 1.  FFT ring only.
enum : int32_t { JOB_MULTI = 0, JOB_DIRECT = 1, JOB_SIGN = 2, JOB_ACC = 3 };
struct DevGate {
    int32_t n_in;
    int32_t offset;  // units of Delta/2 = 2^58
    int32_t in_slot[16];
    int32_t in_w[16];
    int32_t n_out;
    int32_t direct;
    int32_t out_slot[MAX_OUT];
    uint8_t lut[MAX_OUT][16];
};
static_assert(sizeof(DevGate) == 304, "DevGate layout");
// the input side of the affine value cst + w * arena[slot] (cst in units of Delta; slot < 0: the
// constant alone), what a pack row or a linear op reads; outputs and LUTs are left zero
inline DevGate affine_gate(int slot, int w, int cst) {
    DevGate g;
    std::memset(&g, 0, sizeof g);
    g.offset = 2 * cst;
    if (slot >= 0) {
        g.n_in = 1;
        g.in_slot[0] = slot;
        g.in_w[0] = w;
    }
    return g;
}
// a selector job's index: the first four bytes of lut[0], little endian
constexpr int MAX_SELECTORS = 2 * (int)NEEDLE_MAX_CHARS;
FR_HD uint32_t acc_selector(const DevGate& g) {
    return (uint32_t)g.lut[0][0] | ((uint32_t)g.lut[0][1] << 8) | ((uint32_t)g.lut[0][2] << 16) |
           ((uint32_t)g.lut[0][3] << 24);
}
inline void set_acc_selector(DevGate& g, uint32_t q) {
    for (int i = 0; i < 4; ++i) g.lut[0][i] = (uint8_t)(q >> (8 * i));
}
// An extract-sum (private search over clear content, select_sum.hip): the big LWE in out_slot
// is the sum over its terms (selector q, content position pos, half h) of the sample extract
// of selector q at coefficient ((content[pos] >> 4 h) & 15) N/16.  No job: no keyswitch, no rotation.
// Over a byte-table needle (NEEDLE_BYTES: the form is the bound selector table's, bind_selectors)
// a term is (table i, pos, 0): selector i / (N/256) at coefficient (i % (N/256)) 256 + content[pos].
constexpr int SUM_MAX_TERMS = 16;
struct DevSum {
    int32_t out_slot;
    int32_t n_terms;
    int32_t term[SUM_MAX_TERMS][3];  // (q, pos, h)
};
static_assert(sizeof(DevSum) == 200, "DevSum layout");
// sum of squared w_f coefficients of a LUT (noise growth of its factored output)
int lut_w_norm2(const uint8_t* lut);

struct DeviceTimers {
    double br_ms = 0, ks_ms = 0;
    uint64_t br_launches = 0, br_gates = 0, lut_outputs = 0;
    // the part of the above in latency-shape launches (at most one bootstrap per CU)
    double lat_br_ms = 0;
    uint64_t lat_launches = 0, lat_gates = 0;
    // the part in pair-shape launches (k = 1, two bootstraps per workgroup)
    double pair_br_ms = 0;
    uint64_t pair_launches = 0, pair_gates = 0;
};

// The launch shape of a blind rotation, chosen by Device::br_shape from the batch size (FFT
// ring: fft_br.hip, FbrShape; RNS ring: Latency / Throughput pick the lane geometry)
enum class BrShape { LatencyKP, Latency, Dual, Pair, Throughput };

struct ClientKey;
struct RngKey;
class Device;
// arena slots owned by a call, a plan or a handle in the making (owned.h)
using Slots = gpu::SlotsOf<Device>;

// The two forms of a needle: 2 m selectors of 16-entry nibble tables (fr_find* and the clear
// searches), or m 256-entry byte tables, N/256 to a selector (the clear searches only).
enum NeedleForm : int { NEEDLE_NIBBLES = FR_NEEDLE_NIBBLES, NEEDLE_BYTES = FR_NEEDLE_BYTES };
// A needle on the device (private search): its selectors, [selector][polynomial][N] u64.
// Move-only.  Finds on any lane may read it, so, by Plan's rule (plan.h), it waits for every
// lane before its memory goes.
struct DevNeedle {
    gpu::DevBuf<uint64_t> words;
    size_t m = 0;  // characters: 2 m selectors (bytes: m tables in ceil(256 m / N) selectors)
    NeedleForm form = NEEDLE_NIBBLES;
    // what bind_selectors takes as its count: the indices an extract-sum's or a job's first field may take
    size_t tables() const { return form == NEEDLE_BYTES ? m : 2 * m; }
    Device* dev = nullptr;
    DevNeedle() = default;
    DevNeedle(DevNeedle&&) = default;
    DevNeedle& operator=(DevNeedle&&) = delete;
    ~DevNeedle();
};

class Device {
  public:
    Device(const Params& p, int device);
    ~Device();
    Device(const Device&) = delete;
    Device& operator=(const Device&) = delete;

    const Params& params() const { return p_; }
    int device() const { return dev_; }

    // keys: KSK torus 2^64 [i][j][t]; BSK coefficient domain mod Q [i][r][c][coef]
    void upload_keys(const std::vector<uint64_t>& ksk, const std::vector<uint64_t>& bsk);
    bool has_keys() const { return ksk_ && (p_.ring == FR_RING_FFT ? bool(d_fbsk_[0]) : bool(d_bsk_)); }
    // server-key generation on the device (keygen.hip; FFT ring): the same keys
    // as gen_ksk + gen_bsk on the host, bit for bit; the torus keys stay on the
    // device for download_server_key
    // mask_key != nullptr: the compact form (keys.h) -- every kernel runs under the public
    // mask key, `key` only draws the noise on the host and is no kernel argument
    void gen_server_key(const ClientKey& ck, const RngKey& key, const RngKey* mask_key = nullptr);
    // install a compact server key (FFT ring): `bodies` are the blob's KSK bodies
    // [kN * ks_level] then BSK bodies [W][k+1][N] (u64, little endian, any alignment); one
    // H2D copy, the masks expanded from mask_key on the device, then the transforms of
    // gen_server_key.  The torus keys stay on the device for download_server_key.
    void load_server_key_compact(const RngKey& mask_key, const uint8_t* bodies);
    // stages of the last load_server_key_compact under fr_set_profiling, HIP events, ms:
    // H2D copy, k_expand_ksk, k_expand_rows (the BSK), KSK limbs, k_bsk_fourier
    const double* key_load_ms() const { return key_load_ms_; }
    void download_server_key(uint64_t* ksk, size_t ksk_len, uint64_t* bsk, size_t bsk_len);
    // Packing key (keys.h: pk_rows rows of (k+1) N words).  Generated on the device word for
    // word as gen_packing_rows does on the host, or uploaded (little-endian u64 rows, any
    // alignment); both keep the torus rows on the device for download_packing_key and build
    // the byte limbs pack_bools multiplies by.  All three wait for the device.
    // gen_packing_key: the masks under mask_key, which is the kernel's argument, the noise
    // drawn on the host under noise_key (the standard form: one key for both); compact: the
    // compact form (keys.h), mask_key the public mask key and the bodies rounded to 40 bits
    void gen_packing_key(const ClientKey& ck, const RngKey& mask_key, const RngKey& noise_key, bool compact = false);
    void upload_packing_key(const void* rows);
    void download_packing_key(uint64_t* rows);
    // install a compact packing key: `planes` are the blob's high plane u32[3kN][N] then low
    // plane u8[3kN][N] (little endian, any alignment); one H2D copy, one kernel that expands
    // the masks from mask_key and rebuilds the bodies, then the byte limbs
    void load_packing_key_compact(const RngKey& mask_key, const uint8_t* planes);
    // the two planes gathered on the device from the resident rows (pk_compact_planes bytes)
    void download_packing_key_compact(uint8_t* planes);
    // stages of the last load_packing_key_compact under fr_set_profiling, HIP events, ms:
    // H2D copy, expansion, byte limbs
    const double* pk_load_ms() const { return pk_load_ms_; }
    bool has_packing_key() const { return bool(pksk_); }
    // parity hook: column col < (k+1) N of the byte-limb operand recombined into its 3 kN torus words
    void packing_limb_column(int col, uint64_t* out_host);
    // Packing keyswitch (keys.h: pack_host computes the same words): boolean j < n <= N is
    // the affine form gates[j].offset 2^58 + sum_q in_w[q] arena[in_slot[q]] (outputs unused);
    // the (k+1) N words of the packed GLWE are copied to out_host.  Runs on the current lane's
    // stream after whatever wrote the slots; returns after the download.  fr_pack_bools* call it
    // outside a lane, so it runs on lane 0's stream, which first waits for every lane's queued
    // work (cur_stream): packs of results from different lanes serialise behind all lanes.
    // Inside a lane (fr_match_starts_packed) it runs on that lane's stream after the lane's
    // launches, on the lane's own scratch, and waits for that stream only.
    void pack_bools(const DevGate* gates, size_t n, uint64_t* out_host);
    // The same pack in its compact form (keys.h: compress_packed computes the same values): the
    // packed GLWE's k N mask coefficients and its first n body coefficients, each rounded to its
    // top 16 bits by k_pack_compress; only these k N + n u16 values are downloaded.
    void pack_bools_compact(const DevGate* gates, size_t n, uint16_t* out_host /* kN + n */);
    // The pack of n starts that share R <= n rows (keys.h: pack_host_mapped computes the same
    // words): start j < n <= N is boolean rows[map[j]], or the constant 0 where map[j] < 0.  The
    // digits and the GEMM run over the R rows, k_pack_map_sum over the n starts; one of out_words
    // ((k+1) N words) and out_c16 (kN + n values) receives the result as in the packs above.
    // Refused before anything is staged: an entry >= R, a row no start reads, R < 1 (check_pack_map).
    void pack_mapped(const DevGate* rows, size_t R, const int32_t* map, size_t n, uint64_t* out_words,
                     uint16_t* out_c16);
    // HIP-event ms of the last pack under fr_set_profiling: digits (with the zeroing of the
    // scratch), GEMM, rotate-sum, and the compact form's rounding (0 for pack_bools)
    const double* pack_ms() const { return pack_ms_; }
    // fresh encryptions of block messages (encrypt_blocks, keys.h) written into
    // allocated arena slots, bit-identical to the host encryption
    void encrypt_to_slots(const ClientKey& ck, const uint8_t* msgs, size_t count, const RngKey& key, uint64_t first_block,
                          const int* slots);

    // compact content (keys.h): allocates `count` arena slots (returned) and rebuilds block
    // q's LWE in slot q of them -- the masks from mask_key on the device, the body from
    // `bodies` (count u64, little endian, any alignment; copied before the call returns).
    // Lane 0; stream-ordered: returns once enqueued.  The bodies and the slot list travel in
    // one H2D copy from a pinned staging ring owned by the device (no staging allocation per
    // call).
    Slots expand_to_slots(const RngKey& mask_key, uint64_t first_block, const uint8_t* bodies, size_t count);
    // ms of the last expand_to_slots' kernel under fr_set_profiling (HIP events; a profiled
    // call waits for its kernel)
    double expand_ms() const { return expand_ms_; }

    // arena of big-LWE slots
    int alloc_slot();
    void free_slot(int s);
    void write_slots(const int* slots, size_t n, const uint64_t* host /* n * lwe_len */);
    void read_slot(int slot, uint64_t* host /* lwe_len */);
    // packed device-to-device copies of slots (lwe_len u64 each) to / from a device
    // buffer owned by the caller; both synchronise the library's stream on return
    void slots_to_device(const int* slots, size_t n, uint64_t* dst);
    void device_to_slots(const int* slots, size_t n, const uint64_t* src);
    // stream-ordered slots_to_device for n <= 16 (the slot list travels as a kernel
    // argument): returns once enqueued; order other streams after it with an event on stream()
    void slots_to_device_async(const int* slots, size_t n, uint64_t* dst);
    void* stream() const { return cur().stream.get(); }
    void zero_slot(int slot);
    // slots ever handed out (the high-water mark) and the free list's length; a slot whose
    // free is deferred counts as neither until the next sync()
    size_t arena_slots() const { return next_slot_; }
    size_t arena_free_slots() const { return free_slots_.size(); }

    // run one dependency level of gates (all independent), async on the stream
    void run_level(const DevGate* gates, size_t n);
    // the same for a batch already resident on the device (upload_gates); `host`
    // is its host copy (validated when uploaded; read for the profiling counters).
    // n_refs > 0: the batch reads content references (in_slot = -1 - r, r < n_refs)
    // through the content map bound last (bind_content, at least n_refs entries)
    void run_level_resident(const DevGate* d_gates, const DevGate* host, size_t n, size_t n_refs = 0);
    // validated (content references r < n_refs allowed), synchronous; the batch is the
    // caller's (a Plan's: plan.h says when it may go)
    gpu::DevBuf<DevGate> upload_gates(const DevGate* gates, size_t n, size_t n_refs = 0);
    // content map of a template plan: reference r reads arena slot cmap[r] (-1: not
    // read by the plan).  Stream-ordered: launches enqueued after this call see it,
    // launches enqueued before it keep the previous map.
    void bind_content(const int* cmap, size_t n);
    // Private search (FFT ring).  upload_needle: the 2 m expanded selectors (2 m (k+1) N words),
    // one H2D copy, synchronous.  bind_selectors is to a selector launch what bind_content is to
    // a template plan: JOB_ACC jobs enqueued on the current lane after it read selector q < count
    // at table + q (k+1) N (the pointer is a launch argument: launches enqueued before keep
    // theirs).  nullptr: none bound.  A byte-table needle is ceil(256 m / N) selectors of the same
    // (k+1) N words, bound with count = m: its tables are what an extract-sum indexes, and no
    // JOB_ACC job may read it.
    DevNeedle upload_needle(const uint64_t* words, size_t m, NeedleForm form = NEEDLE_NIBBLES);
    void bind_selectors(const uint64_t* table, size_t count, NeedleForm form = NEEDLE_NIBBLES);
    // Private search over clear content (select_sum.hip).  bind_text: the call's n content bytes,
    // copied before it returns and bound to the current lane in stream order through the lane's
    // staging ring, as bind_content binds a map.  run_sums / run_sums_resident: one launch of n
    // extract-sums over the selector table and the content bound last on the current lane, every
    // index checked against both bounds first; staged descriptors (lane 0 only) or a batch
    // already resident (upload_sums: validated, synchronous; the batch is a Plan's).
    void bind_text(const uint8_t* text, size_t n);
    void run_sums(const DevSum* sums, size_t n);
    void run_sums_resident(const DevSum* d_sums, const DevSum* host, size_t n);
    gpu::DevBuf<DevSum> upload_sums(const DevSum* sums, size_t n);
    // linear combination without bootstrap (NOT of a boolean): out = offset*2^58 + sum w*in
    void run_linear(const DevGate& g);
    void sync();

    // Lanes (serving without key copies): lane 0 is the stream above; lanes 1..n are
    // further streams of this device with their own keyswitch / digit scratch and content
    // map, sharing the keys and the arena.  Between enter_lane(i) and leave_lane() every
    // launch goes to lane i's stream, ordered after everything enqueued on lane 0 so far.
    // Work on lane 0 waits (device-side, by event) for every lane's enqueued work before it
    // runs; slots freed while a lane may still read them return to the free list only after
    // a host synchronisation of every lane (sync()).
    void set_lanes(int n);                                 // n = 1: lane 0 only; n >= 2: lanes 1..n beside it
    int match_lanes() const { return (int)lanes_.size(); }  // lanes asynchronous matches go to
    void enter_lane(int i);
    void leave_lane();
    void set_profiling(int level) { profiling_ = level; }
    DeviceTimers& timers() { return timers_; }

    // single-stage entry points for parity tests
    void keyswitch_host(const uint64_t* in, size_t count, uint64_t* out);
    void blind_rotate_host(const uint64_t* ks_in, const uint8_t* luts, size_t count, uint64_t* out);
    // one job with n_out LUTs on one keyswitched input (multi-value or direct)
    void blind_rotate_multi_host(const uint64_t* ks_in, const uint8_t* luts, int n_out, int direct, uint64_t* out);
    // one selector launch: job i starts from the GLWE ciphertext accs + i (k+1) N
    void blind_rotate_acc_host(const uint64_t* ks_in, const uint64_t* accs, size_t count, uint64_t* out);
    void ring_mul_host(const uint64_t* a, const uint64_t* b, size_t count, uint64_t* out);
    // the extract-sum kernel alone: sum i has n_terms[i] terms, 3 words each (q, pos, h), one
    // after the other in `terms`; lwe_len words per sum to `out`.  Lane 0, synchronous.
    void select_sum_host(const DevNeedle& needle, const uint8_t* text, size_t len, const int32_t* terms,
                         const int32_t* n_terms, size_t n, uint64_t* out);
    // ms of the last select_sum_host's kernel under fr_set_profiling (HIP events)
    double select_sum_ms() const { return select_sum_ms_; }
    // repeated full-PBS batches on resident inputs (bench / roofline)
    void bench_pbs(const std::vector<DevGate>& gates, int iters, double* br_ms, double* total_ms);

    std::string info() const;

  private:
    // Everything a lane owns.  Lane 0 is lane0_, lanes 1..n are lanes_; cur() is the one
    // launches go to.  The stream is declared first: it outlives what is used on it.
    struct LaneState {
        gpu::Stream stream;
        gpu::DevBuf<uint64_t> ks;    // keyswitch outputs [gates][ks_stride]
        gpu::DevBuf<int8_t> dig;     // keyswitch digits [rows][kN*ks_level]
        gpu::DevBuf<DevGate> pk_gates;  // pack_bools: the booleans' descriptors
        gpu::DevBuf<int8_t> pk_dig;  // pack_bools: digits [rows][3 kN], allocated at the first pack
        gpu::DevBuf<uint64_t> pk_g;  // pack_bools: keyswitched rows [n][(k+1) N], then the packed GLWE
        gpu::DevBuf<uint16_t> pk_c16;  // pack_bools_compact: the k N + N rounded coefficients
        gpu::DevBuf<int32_t> pk_map;   // pack_mapped: the row of each start, N entries
        // key products of the lane's smallest launches [bootstrap][step][P][own, other][m][lane]
        // (fft_br.hip: k_key_products), allocated at the first such launch, grown to the largest
        gpu::DevBuf<double> kpre;
        gpu::StagingRing<int> cmap;  // content map (bind_content)
        size_t cmap_n = 0;           // entries bound
        const uint64_t* sel = nullptr;  // selector table (bind_selectors)
        size_t sel_n = 0;               // selectors bound (bytes: tables)
        NeedleForm sel_form = NEEDLE_NIBBLES;
        gpu::StagingRing<uint8_t> text;  // clear content bytes (bind_text)
        size_t text_n = 0;               // bytes bound
        gpu::Event done_ev;          // recorded on the lane's stream when it is left
        bool pending = false;        // work enqueued since lane 0 last waited for it
    };
    // The lanes come before every other resource, so their streams are destroyed last.
    LaneState lane0_;
    std::vector<LaneState> lanes_;  // lanes 1..n
    int lane_ = 0;                  // current lane
    LaneState& cur() { return lane_ ? lanes_[lane_ - 1] : lane0_; }
    const LaneState& cur() const { return lane_ ? lanes_[lane_ - 1] : lane0_; }
    bool lanes_pending_ = false;
    bool lanes_unsynced_ = false;   // lane work not yet host-synchronised (deferred frees)
    gpu::Event main_ev_;            // lane 0's progress, waited for by a lane on entry
    std::vector<int> deferred_free_;
    // the stream of the current lane; on lane 0 it first waits (device-side) for the lanes
    hipStream_t cur_stream();
    void join_lanes();
    void sync_all();  // host-synchronise every lane, recycle the deferred slots
    void ensure_arena(size_t slots);
    void ensure_ks(size_t n);     // the current lane's keyswitch scratch for n gates
    void ensure_gates(size_t n);  // the gate ring for n descriptors
    void validate_gates(const DevGate* gates, size_t n, size_t n_refs = 0) const;
    void launch_level(const DevGate* d_gates, const DevGate* host, size_t n);
    // profiling: per-level event triples resolved at sync() (no sync per level)
    gpu::Event take_event();
    void resolve_timers();
    void ensure_digits(size_t rows);
    // A keyswitching key (LWE: ksk_, packing: pksk_): the torus rows [KD][ncols] (export, VALU
    // keyswitch) and their balanced byte limbs in fragment order, the MFMA GEMM's column operand
    struct LimbKey {
        gpu::DevBuf<uint64_t> rows;
        gpu::DevBuf<int8_t> limbs;       // [col*8 + limb][k], nlc limb columns (build_limbs, keyswitch.hip)
        int KD = 0, ncols = 0, nlc = 0;  // nlc: ncols * 8 padded to whole 4-wave column groups
        explicit operator bool() const { return rows && limbs; }
        void alloc_rows(int kd, int nc) {  // the shape and fresh rows; no limbs until build_limbs
            limbs.reset();
            KD = kd, ncols = nc, nlc = ((nc * 8 + 127) / 128) * 128;
            rows.alloc((size_t)kd * nc);
        }
        void reset() { rows.reset(), limbs.reset(); }
    };
    void build_limbs(LimbKey& key);
    // every buffer of an installed key; the installs drop under a Replacing guard (device_impl.h)
    void drop_server_key() {
        ksk_.reset(), d_tbsk_.reset(), d_bsk_.reset(), d_fbsk_[0].reset(), d_fbsk_[1].reset();
        lane0_.kpre.reset();
        for (auto& l : lanes_) l.kpre.reset();
    }
    void drop_packing_key() { pksk_.reset(); }
    // MFMA keyswitch of n rows: row tiles per wave and n padded to whole tiles of them (ks_shape);
    // column tiles per wave, the LDS-DMA ring (k_ks_glds: MR 4, MC 1 only) and K slices: the caller's
    struct KsShape {
        int MR;
        size_t padded;
        int MC = 1, GZ = 1;
        bool lds = true;
    };
    KsShape ks_shape(size_t n) const {
        const int MR = n >= ks_mr4_min_ ? 4 : 1;
        return {MR, (n + 32 * MR - 1) / (32 * MR) * (32 * MR)};
    }
    // its two launches (keyswitch.hip): digits of the gadget (2^KSB, KSL) into dig, out's columns
    // < out_n zeroed and the body in column out_n; then out -= dig x key.limbs.
    // ev_start / ev_stop (profiling): HIP events stamped by the kernels' own dispatch
    // (hipExtLaunchKernel) -- the first kernel's start and the last one's end -- so timing
    // adds no marker packets between dependent launches (each cost ~5 us of gap)
    template <int KSB, int KSL>
    void launch_ks_digits(const DevGate* d_gates, size_t n, size_t padded, int8_t* dig, uint64_t* out, int out_n,
                          int out_stride, hipEvent_t ev_start);
    void launch_limb_gemm(const int8_t* dig, const LimbKey& key, size_t n, const KsShape& sh, uint64_t* out,
                          int out_stride, hipEvent_t ev_stop);
    void launch_ks(const DevGate* d_gates, size_t n, uint64_t* d_ks, hipEvent_t ev_start = nullptr,
                   hipEvent_t ev_stop = nullptr);
    // acc: a launch of selector jobs (JOB_ACC) only; else none of them
    void launch_br(const DevGate* d_gates, const uint64_t* d_ks, size_t n, hipEvent_t ev_start = nullptr,
                   hipEvent_t ev_stop = nullptr, bool acc = false);
    // selector jobs come first in a batch: their count, checked against the table bound
    size_t leading_selector_jobs(const DevGate* host, size_t n) const;
    void launch_jobs(const DevGate* d_gates, const DevGate* host, size_t n, bool acc);  // one keyswitch + rotation
    void run_br_jobs(const uint64_t* ks_in, std::vector<DevGate>& gates, uint64_t* out);  // the blind_rotate_*_host hooks
    // select_sum.hip
    void validate_sums(const DevSum* sums, size_t n, size_t n_sel, size_t text_n,
                       NeedleForm form = NEEDLE_NIBBLES) const;
    void check_sums(const DevSum* host, size_t n) const;  // against what the current lane has bound
    void launch_select_sum(const uint64_t* table, const DevSum* d_sums, size_t n);
    gpu::StagingRing<DevSum> sums_;  // staged extract-sums (lane 0), as gates_
    double select_sum_ms_ = 0;
    // FR_RING_RNS (rns_br.hip)
    void init_rns();
    void upload_rns_bsk(const std::vector<uint64_t>& bsk);
    void launch_br_rns(const DevGate* d_gates, const uint64_t* d_ks, size_t n, hipEvent_t ev_start, hipEvent_t ev_stop);
    void init_ks();  // keyswitch.hip: the FR_KS_* settings
    // FR_RING_FFT (fft_br.hip)
    void init_fft();
    void upload_fft_bsk(const std::vector<uint64_t>& bsk);
    void launch_br_fft(const DevGate* d_gates, const uint64_t* d_ks, size_t n, hipStream_t stream,
                       hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, bool acc = false);
    void build_fourier_bsk();  // keygen.hip: d_fbsk_ (every lane layout in use) from d_tbsk_
    double key_load_ms_[5] = {0, 0, 0, 0, 0};
    double pk_load_ms_[3] = {0, 0, 0};
    // expand_to_slots: the bodies and the slot list of a call, one copy (lane 0)
    gpu::StagingRing<uint8_t> xstage_;
    double expand_ms_ = 0;
    void stage_slot_list(const int* slots, size_t n);  // -> d_slot_list_ (stream order)
    gpu::DevBuf<int> d_slot_list_;

    Params p_;
    int dev_;
    int e_ = 8;        // residues per lane in the NTT kernels (8 or 16; measured: 8 wins for k=1 and k=2)
    int e_small_ = 8;  // ... for launches of at most small_batch_ bootstraps
    size_t small_batch_ = 256;
    LimbKey ksk_;                   // LWE keyswitch key: kN ks_level rows of n + 1 words
    gpu::DevBuf<uint64_t> d_tbsk_;  // torus BSK of a device-generated or device-expanded key (export)
    LimbKey pksk_;                  // packing key: 3 kN rows of (k+1) N words (pack_bools)
    double pack_ms_[4] = {0, 0, 0, 0};
    // both forms of the pack: the words to out_words, or (out_c16) the rounded values alone
    // (R rows, n starts; map NULL: start j reads row j and R == n)
    void pack_launch(const DevGate* gates, size_t R, const int32_t* map, size_t n, uint64_t* out_words,
                     uint16_t* out_c16);
    int pk_split_ = 0;              // FR_PK_SPLIT: K slices of the packing GEMM (a divisor of 24; 0: auto)
    bool ks_mfma_ = true;         // FR_KS_MFMA=0: the VALU lincomb+keyswitch kernel
    size_t ks_mr4_min_ = 96;      // FR_KS_MR4_MIN: batches from this size use 4 row tiles per wave (k_ks_glds; ab_ks_glds.log: 100 gates 44 -> 37 us, 64 gates no gain)
    int ks_mc_ = 0;               // FR_KS_MC=2: two column tiles per wave in the 4-row-tile shape (else one)
    int ks_split_ = 0;            // FR_KS_SPLIT: K slices (a divisor of kN*ks_level/256; 0: auto)
    int ks_xcd_ = 1;              // FR_KS_XCD=0: plain workgroup order of the MFMA keyswitch (k_ks_mfma)
    bool ks_dig16_ = true;        // FR_KS_DIG16=0: the digit pass with byte stores (k_ks_digits)
    bool ks_lds_ = true;          // FR_KS_LDS=0: four-row-tile keyswitch without the LDS-DMA ring (k_ks_mfma<4, 1>)
    gpu::DevBuf<uint32_t> d_bsk_;  // NTT domain [i][r][c][prime][slot], Montgomery form, scaled by 1/N
    gpu::DevBuf<uint32_t> d_tw_;   // Montgomery zeta per prime [2][N]
    // FR_RING_FFT: Fourier BSK [w][r][c][m][lane] (complex f64, scaled by 1/M), twiddles,
    // psi quadrant table, leaf exponents (fft.h)
    int fft_e_ = 4;           // complex points per lane in the throughput shape (4 or 8)
    size_t fft_small_ = 256;  // launches of at most this many bootstraps use the latency shape
    // k = 1: larger launches up to this many use the pair shape (2 per workgroup; every size
    // by default: profiles/r03/ab_pair_shape.log)
    size_t fft_pair_ = SIZE_MAX;
    bool fft_dual_ = false;  // FR_FFT_DUAL=1: the dual shape instead of the pair (experiment)
    // k = 1: latency-shape launches of at most this many bootstraps precompute their key
    // products on the idle CUs (k_key_products, then k_blind_rotate_fft_kp); FR_FFT_KPRE_BATCH,
    // 0: off.  24.3 MB of scratch per bootstrap and lane.  32: the largest of 1, 2, 4, ..., 64 at
    // which every run of the pair of kernels beats the plain latency shape (1.19 against 1.34 ms;
    // at 64 1.5-2% at the median for 1.6 GB of scratch: profiles/key_products/)
    size_t fft_kpre_ = 32;
    // Fourier BSK, one copy per lane geometry in use: [0] E = 4 (latency shape, always),
    // [1] E = 8 (the throughput shape's when fft_e_ is that)
    gpu::DevBuf<double> d_fbsk_[2];
    static int fbsk_index(int E) { return E == 4 ? 0 : 1; }
    bool fbsk_needed(int E) const { return E == 4 || E == fft_e_; }
    gpu::DevBuf<double> d_ftw_;
    gpu::DevBuf<double> d_fqt_;   // psi^k, k < 2N
    gpu::DevBuf<uint16_t> d_fleaf_;
    gpu::DevBuf<uint64_t> d_arena_;  // [slots][slot_stride]
    std::vector<int> free_slots_;
    size_t next_slot_ = 0;
    // gate descriptors of a staged level (lane 0: lanes run resident plans only); no
    // stream-wide sync between levels
    gpu::StagingRing<DevGate> gates_;
    struct PendingTimer {
        gpu::Event ev[4];  // KS start, KS end, BR start, BR end
        size_t gates, outs;
        bool lat, pair, ks;
        bool chain;  // BR timed from the keyswitch's end event (no start event on the BR launch)
        void count_as(BrShape shape);  // lat / pair: the timers' per-shape sums
    };
    BrShape br_shape(size_t n, bool acc) const;  // launch_br's shape choice for n bootstraps (acc: selector jobs)
    std::vector<PendingTimer> pending_;
    std::vector<gpu::Event> event_pool_;
    int profiling_ = 0;  // fr_set_profiling level
    bool timer_chain_ = true;  // level 1: stop events only (FR_TIMER_CHAIN=0: start + stop on the BR launch)
    DeviceTimers timers_;
    gpu::Event ev_[4];  // bench_pbs
};

}  // namespace fr
