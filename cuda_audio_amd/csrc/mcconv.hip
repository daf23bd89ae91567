// mcconv.hip — engine state + the C ABI of include/mcconv.h.
//
// One mc_engine corresponds to one reference `Convolution` object
// (conv.h:30-86): it owns the IR bank (_irBuffers, conv.h:77), the
// frequency-domain delay line that replaces the reference's whole-IR spectra
// and N-long overlap-add accumulator (conv.h:72-75), the per-half parameters
// (cc[2].value, conv.h:33-50) and the running-mean timer (conv.h:61,79-80).
#include <hip/hip_runtime.h>
#include <immintrin.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/mcconv.h"
#include "owned.h"
#include "params_handoff.h"
#include "kernels.hip.h"
#include "ossave.hip.h"
#include "singlefft.hip.h"
#include "resample.hip.h"
#include "irshape.hip.h"
#include "ireq.hip.h"
#include "irdamp.hip.h"
#include "irdecay.hip.h"
#include "irplate.hip.h"
#include "irspring.hip.h"
#include "irroom.hip.h"
#include "irsynth.hip.h"
#include "irsweep.hip.h"
#include "irfloor.hip.h"
#include "irdensity.hip.h"
#include "iriacc.hip.h"
#include "irsti.hip.h"
#include "irresponse.hip.h"
#include "irtail.hip.h"
#include "irphase.hip.h"
#include "irfilter.hip.h"
#include "irmatch.hip.h"
#include "irparts.hip.h"

// Environment switches, read at mc_create.  The library reads fourteen.  Ten select paths a caller can also reach through
// mc_config or that the tests compare bit for bit:
//   MCCONV_FORM, _OS, _FFT2, _FFT2_FUSED, _FFA_LEVELS  which form sums the partitions
//   MCCONV_TD_FFT                                      Q8 cut terms in the time domain
//   MCCONV_NO_PARK, _PARK_MS, _NO_SPIN, _BAR_IO        the JACK path's waiting and I/O
// Four are test hooks that make a path of the library reachable at test sizes:
//   MCCONV_OS_MIN        shortest batch that takes the overlap-save form (mc_engine::os_min_blocks)
//   MCCONV_FFT2_WORK     blocks x partitions from which a batch takes the fused second-level form (mc_engine::fft2_work)
//   MCCONV_TAIL_FORM     td | fd: one form for every 256-frame JACK tail (mc_engine::tail_form)
//   MCCONV_SF_STOCKHAM   single-transform form: pass 2 of the inverse through the LDS transform at every size (SfState::stockham)

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(MC_ERR_HIP, "%s -> %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

constexpr int kMaxIrs = 256;
constexpr int kMixIrs = 4;  // merged spectra of deselected IRs: [half][buffer], table entries kMaxIrs ..
constexpr int kStageBufs = 4;
constexpr int kEvPool = KernelTiming::kPool;
constexpr int kPipe = 2;
constexpr int kStampSlots = 64;  // timed launches between two drains whose kernels leave their own time stamps
constexpr int kNchunk = 2;       // partition chunks of the streaming MAC: its workgroups per (bin, block)
// fp16 storage: the exponent of an IR's power-of-two scale16 goes no higher, so that scale16 * FDL16_SCALE (<= 2^126) and its
// reciprocal (>= 2^-126), which the streaming MAC multiplies into the gains, stay normal floats however quiet the IR (without it
// an IR whose largest spectrum entry is below 2^-115 got scale16 = inf and an inverse of zero).  At the limit the inverse is
// 2^-126, so its product with any gain below 1 (mac_stream_body, g * inv) is a SUBNORMAL float: the sum of such an IR is right
// only because this build keeps fp32 subnormals (hipcc's default for gfx9; -fgpu-flush-denormals-to-zero would silence the IR).
// tests/test_gpu_fp16_storage.py::test_quiet_ir runs that case at a wet gain of 0.3.  A lower limit would keep the product
// normal but push the IR's own halves into the subnormal range instead; an IR this quiet gives up precision either way
constexpr int kScale16MaxExp = 122;
constexpr int kG2Pmax = 5632;    // longest block-axis convolution (partitions) the fused 8192-point form takes: measured crossover
                                 // with the split 16384-point form ~5700 (30 s IRs, P = 5168: 0.25 vs 0.27 ms for a third more blocks)

inline uint32_t next_pow2(uint64_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

inline double pan_l(double p) { return p >= 0 ? 1 - p : 1; }  // conv.cu:386
inline double pan_r(double p) { return p <= 0 ? 1 + p : 1; }  // conv.cu:387

// What mc_ir_shape_info, _damp_info, _synth_info, _sweep_info, _tail_info, _phase_info, _filter_info, _match_info, _parts_info, _room_info, _room_mics_info, _room_bands_info, _room_head_info, _plate_info and _spring_info report of an IR's last
// load: one entry per kind, on when that load had the step or the source (a shape with something on, an eq band or damping count as a shape, and
// so do a synthesised, a swept and a tailed load), with the numbers the getter hands out (include/mcconv.h says what they are)
enum IrFactKind { FACT_SHAPE, FACT_DAMP, FACT_SYNTH, FACT_SWEEP, FACT_TAIL, FACT_PHASE, FACT_FILTER, FACT_MATCH, FACT_PARTS, FACT_ROOM, FACT_ROOM_MICS, FACT_ROOM_BANDS, FACT_ROOM_HEAD, FACT_PLATE, FACT_SPRING, FACT_KINDS };
struct IrFact {
    bool on = false;
    double v[24] = {};
};

struct IrEntry {
    DevArray<float4> d_H;
    DevArray<float4> d_Hp[3];                       // fast-FIR components of the partition sequence: 3 / 9 / 27 arrays,
    bool hp_valid[3] = {false, false, false};       // built on the first batch that selects that level (ensure_hp)
    DevArray<float2> d_H2;  // second-level spectra [2 ch][257 rows][F2_N], built on first use (k_fft2_ir)
    bool h2_valid = false;
    DevArray<float2> d_G2;  // second-level spectra for the fused 8192-point form [2 ch][257 rows][G2_N]
    bool g2_valid = false;
    DevArray<float2> d_h;  // time-domain taps {L, R} (Q8 pass)
    DevArray<float4> d_Htail;  // Q8 pass, frequency-domain form: the last partitions' spectra partition-major [P - tail_p0][256] (ensure_htail)
    int tail_p0 = 0;
    bool tail_valid = false;
    DevArray<float2> d_S;   // single-transform form (mc_config.form = 1): [H_L | H_R], n_ref / 2 bins each
    DevArray<uint2> d_H16;  // fp16 copy of the spectra, scaled by scale16 (precision = fp16)
    float scale16 = 1.f;
    uint64_t taps = 0;
    int P = 0;
    double sums[4] = {0, 0, 0, 0};
    IrFact facts[FACT_KINDS];  // what the last load went through (note_load), for the mc_ir_*_info getters
    std::vector<double> match_curve;  // with FACT_MATCH: hz[J], (before L, R)[J], (gain L, R)[J] (mc_ir_match_curve)
};

}  // namespace


struct BatchCtx {
    int T = 0;
    uint64_t t0 = 0;
    int pstride = 1;
    uint64_t predelay = 0;
    VoiceSums vs;
    int vir[2][MC_MAXV];  // IR index per half and voice (-1 = none)
    int slot = 0;
    int first = 0, count = 0;  // output blocks this engine finishes (the whole batch unless block-sliced)
    int need_a0 = 0, need_a1 = 0, need_b0 = 0;  // blocks the front half transformed: [a0, a1) and [b0, T)
    uint64_t win0 = 0;         // first absolute sample whose segments the front half computed
    bool wet_ready = false;    // the front half overlap-added the window into the wet ring (k_inv_wet)
    bool corr_done = false;    // the Q1/Q2 prefix sums of the batch are final (they rode along with the front half's launches)
    bool drop_done = false;    // Q8 regime: the front half summed the cut terms of the whole batch into d_dropbuf (k_drop_fft)
    int out_from = -1;         // >= 0: the front half finished the output of blocks >= out_from itself (k_inv_wet<true>)
};

// One voice as the MAC sees it
struct ActiveVoice {
    int v;                 // gain-table row
    const IrEntry *ir0, *ir1;
    int p_end;             // partitions to sweep (multiple of 16), before sharding
    bool uniform;          // every slot of the window carries the same gains
    float4 ugain;
};

// Sample the parameters, advance the cross-fade, stage the per-block table of a
// batch of T blocks starting at block t_front, and describe the batch in `ctx`.
struct Staged {
    BatchCtx ctx;
    BlockParams* d_ptab;  // view: this batch's half of mc_engine::d_ptab
    float4* d_sums;       // view: this batch's half of mc_engine::d_sums
    BlockParams first;  // host copy of the first block's parameters
    ActiveVoice act[MC_MAXV];
    int nact = 0;
};


// JACK path: a period launched one call ahead, parked on its doorbell (process_one)
struct JackPre {
    bool valid = false;
    uint64_t block = 0;   // the block it will finish
    unsigned seq = 0;     // its doorbell / completion value
    mc_cc_value cc[2];    // the parameters it was staged with
    Staged st;
    int pm = 1;           // blocks per period it was staged for
    bool carries_sweep = false;  // its kernel also runs the sweep of block + 1 ...
    int carried_vir[2];          // ... for this IR pair
};

// state of the single-transform form (singlefft.hip.h / singlefft_host.hip.h)
struct SfState {
    int N = 0, M = 0, AT = 1;
    DevArray<float2> d_live;  // [half][ch][N/2] live IR spectra (the reference's irFFT, conv.h:72); bin d + M c at [d][c]
    DevArray<float2> d_W;     // [M][512] packed output spectrum
    DevArray<float2> d_T;     // [512][M] between the inverse passes; IR preparation: the packed taps, then U
    DevArray<float2> d_Z;     // [N] IR preparation
    DevArray<float> d_acc;    // [ch][N] accumulators (conv.h:74 residual): a ring, `base` = slot of the next output frame
    DevArray<unsigned> d_ctr;
    unsigned base = 0;
    DevArray<float> d_io[4];  // staging of host-buffer batches, Tmax blocks each
    size_t lds_bytes = 0;
    bool stockham = false;  // MCCONV_SF_STOCKHAM: pass 2 of the inverse through the LDS transform whatever the size
};

struct mc_engine {
    mc_config cfg;
    int device = 0;
    std::unique_ptr<SfState> sf;  // != null: the engine runs the reference's single-transform form (singlefft.hip.h)
    Stream own_stream;
    hipStream_t stream = nullptr;  // view: own_stream, or the caller's (mc_set_stream)
    int Tcap = 0;  // blocks the scratch buffers and rings are sized for: >= Tmax, and enough to re-render history in few launches
    int Tmax = 0, Pcap = 0, Pstride = 0, ring = 0, sr = 0, wr = 0, rc = 0, Tstream = 0;
    int stream_threshold = 0;
    int pm = 1;  // blocks per reference call (JACK period / 256): 1, 2 or 4
    IrEntry irs[kMaxIrs + kMixIrs];
    int mix_buf[2] = {0, 0};  // which of its two merged-IR entries half i used last
    int nirs = 0;

    DevArray<uint2> d_fdl16;  // fp16 mirror of the delay line (precision = fp16)
    bool half = false;
    float4* d_Yc = nullptr;  // view of d_Ycbuf[0], pipelined: of the batch parity's: [256][Tcap] partition sums combined from the fast-FIR components
    DevArray<float2> d_stash;  // second-level transform: spectra parked between the transforms and the products
    // Pipelined batches (mc_config.pipeline): the inverse transforms and the post stage of batch k run on a second
    // stream under the MAC of batch k + 1.  Scratch that both touch is double-buffered by batch parity.
    bool pipelined = false;
    Stream post_stream;
    Event ev_mac[2][2], ev_corr[2], ev_post[2];
    bool post_pending[2] = {false, false};
    DevArray<float4> d_Ybuf[2], d_Ycbuf[2], d_partbuf[2];
    DevArray<float4> d_tailbuf[2];  // chunk partials of the last 2^levels blocks (fast-FIR form)
    float4 *d_Y = nullptr, *d_tail = nullptr, *d_part = nullptr;  // views of d_Ybuf[0], d_tailbuf[0], d_partbuf[0] (pipelined: of the batch parity's)
    DevArray<float4> d_fdl, d_slotgain, d_sums;
    DevArray<float> d_seg, d_wet;
    DevArray<double> d_cring;
    DevArray<double> d_wring;  // [rc][4] window sums per block of an overlap-save batch (k_out_windows), indexed like d_cring
    DevArray<double> d_ctot;   // [ceil(Tmax/256)][4] chunk totals of the Q1/Q2 prefix sums
    // predelay epochs: what blocks played under earlier predelays still owe, by absolute output sample
    DevArray<float> d_res_mac, d_res_fix;  // [2][rr] each
    int rr = 0;
    uint64_t res_end = 0;     // the rings hold output samples < res_end
    uint64_t epoch_b0 = 0;    // first block of the live epoch
    uint64_t cur_delay = 0;   // its predelay
    DevArray<float> d_xhist;   // [2][xr] input history (Q8 pass)
    DevArray<float4> d_gring;  // [MC_MAXV][rc] wet gains of past blocks (Q8 pass)
    int xr = 0;
    DevArray<BlockParams> d_ptab;
    DevArray<float2> d_tw;
    DevArray<float> d_io[4];  // in1, in2, outL, outR staging for host-pointer calls
    int Thost = 0;                                          // blocks per chunk of a host-buffer batch staged through h_io
    // host-buffer batches whose buffers are pinned (mc_host_alloc, hipHostMalloc, hipHostRegister): chunks of Tdev blocks,
    // H2D and compute on two streams, the output stored straight into the caller's buffers; input staging (three sets)
    // made by the first such batch
    std::unique_ptr<PinnedStaging> pinned;
    int Tdev = 0;
    PinnedArray<float> h_io;       // pinned mirror of d_io, 4 * Thost * 256 (mapped, zero-copy: h_io.dev())
    PinnedArray<unsigned> h_flag;  // completion word of the single-period path (mapped)
    unsigned flag_seq = 0;
    DevArray<unsigned> d_done_ctr;  // workgroups of the period's last kernel that have finished
    bool spin_wait = true;
    PinnedArray<BlockParams> h_ptab[kStageBufs];
    Event ptab_ev[kStageBufs];
    bool ptab_ev_used[kStageBufs] = {false, false, false, false};
    int ptab_next = 0;

    // parameters: written by any thread (mc_set_params, mc_handle_cc), sampled at the start of a process call without a
    // lock (params_handoff.h); last_gen = the generation of the pair the last process call ran on (mc_debug_read item 7)
    ParamHandoff ph;
    uint64_t last_gen = 0;

    // Cross-fade state.  The reference keeps live spectra irFFT_i and pulls them towards
    // wet_i * H_sel_i every block: irFFT += (wet H_sel - irFFT)/(vsteps+5) (conv.cu:27, 339-353).
    // irFFT_i is therefore always sum_j c_ij H_j with c_ij <- c_ij (1 - 1/(v+5)) + [j == sel_i] wet_i/(v+5):
    // one coefficient per IR that has been selected recently.  coef[i][v] is that coefficient for
    // the IR in voice slot v of half i.
    struct VoiceSlot {
        int ir = -1;           // IR index, -1 = free
        double coef = 0.0;
        uint64_t last_nz = 0;  // last block whose gain for this slot was non-zero
        bool ever = false;
    } voice[2][MC_MAXV];
    float last_g[MC_MAXV][4];
    uint64_t gain_change_block[MC_MAXV] = {0, 0, 0};  // block at which voice v's gains last changed
    uint64_t last_nz_voice[MC_MAXV] = {0, 0, 0};
    bool voice_ever[MC_MAXV] = {false, false, false};

    uint64_t t_abs = 0;    // blocks finished (front + back done)
    uint64_t t_front = 0;  // blocks whose front half (FFT, MAC, inverse, overlap-add) has been issued
    // up to kPipe batches may sit between their front and back halves (sharded
    // operation overlaps the cross-GPU reduce of batch k with the MAC of batch k+1)
    typedef ::BatchCtx BatchCtx;
    BatchCtx pipe[2];
    int pipe_head = 0, pipe_count = 0;
    uint64_t batch_seq = 0;
    // speculative MAC of the next single block (partitions >= 1 do not depend on the next input)
    bool spec_valid = false;
    // Q8 regime, JACK path: the cut terms a parked launch summed for the period after its own (SweepArgs.drop_next): valid for that block while
    // predelay, epoch and the voices' IRs are what they were (everything else they depend on is at least n_ref frames old)
    struct DropSpec {
        bool valid = false;
        uint64_t block = 0, predelay = 0, epoch_b0 = 0;
        int vir[2][MC_MAXV];
        const float* buf = nullptr;  // view: the d_drop buffer that launch wrote
    } dspec;
    uint64_t spec_block = 0;
    int spec_vir[2][MC_MAXV];
    int spec_nact = 0;
    Event ev_tail;
    DevArray<float4> d_part_jack[2];  // JACK path: the sweep's partials, double-buffered by block parity
    bool td_fft = true;                           // Q8 regime, batches: the cut terms in the frequency domain (MCCONV_TD_FFT=0: time-domain tiles)
    DevArray<float2> d_dropbuf;                   // batches, Q8 regime: the cut terms of a batch's blocks [Tmax][256] {L, R} (k_drop_fft), allocated by the first such batch
    DevArray<float> d_drop[2];                    // JACK path, Q8 regime: a period's tail-drop terms [2][1024] (k_drop_period), by period parity
    JackPre pre;                     // the period parked one call ahead
    bool park = true;                // MCCONV_NO_PARK=1: every period launched when it arrives
    unsigned long long park_ticks = 10000000ull;  // a parked tail gives up after this many 100 MHz ticks (100 ms; MCCONV_PARK_MS)
    unsigned long long* h_bell = nullptr;         // view into h_flag: {sequence number, command} the parked tail polls
    unsigned long long* hd_bell = nullptr;        // view into h_flag.dev(): the same words as the device sees them
    // JACK path on a large-BAR system: doorbell and period input live in fine-grained DEVICE memory that the CPU writes
    // straight through the BAR (posted writes), so the parked tail polls and reads locally instead of over PCIe
    // (MCCONV_BAR_IO=0: mapped host memory as before).  16 floats = the doorbell's line, then in1, in2 (room for 1024 frames each).
    DevArray<float> d_bar;
    bool bar_io = false;
    // Tagged I/O of the 256-frame JACK path (TailArgs::in_gran / out_gran): input granules at byte 16384 of d_bar, output granules
    // in mapped host memory.  On where the BAR path is.
    bool tio = false;
    PinnedArray<unsigned long long> h_gran;   // [2][256] output granules {value, sequence number}
    unsigned* h_exited = nullptr;                 // view into h_flag: sequence number of a parked tail that gave up on its own
    unsigned* hd_exited = nullptr;                // view into h_flag.dev()
    // how often a parked period was used / gave up on its own (host away > park_ms) / was told to give up: mc_debug_read item 6
    uint64_t n_park_hit = 0, n_park_timeout = 0, n_park_cancel = 0;
    DevArray<unsigned> d_tailform;  // 256-frame tails by the form partition 0 took {frequency domain, time domain}, counted by the kernel (mc_debug_read item 16)
    int tail_form = 0;               // MCCONV_TAIL_FORM=td|fd: one form for every 256-frame tail (0: the first look decides)
    uint64_t n_drop_carried = 0;  // JACK path, Q8 regime: periods whose cut terms came with the launch before theirs (mc_debug_read item 9, fourth word)
    uint64_t n_mac_form[3] = {0, 0, 0};  // batches whose partition sums took the fused / split second-level transform / the resident MAC (form_counter; mc_debug_read item 10)
    uint64_t n_drop_fft = 0, n_drop_ahead = 0, n_drop_tiles = 0;  // Q8 regime: batches by the form their cut terms took (mc_debug_read item 9)
#ifdef MC_JACK_TRACE
    double tr_launch = 0, tr_flag = 0, tr_total = 0, tr_kernel = 0, tr_gap = 0, tr_out = 0, tr_clk = 0, tr_c[3] = {0, 0, 0};
    unsigned long long tr_prev_end = 0;
    long tr_n = 0;
#endif
    bool fft2 = true;     // long batches: second-level transform along the block axis instead of the MAC
    bool fft2_fused = true;  // ... in the fused 8192-point form where it applies
    int64_t fft2_work = 300000;  // blocks x partitions from which a batch takes the fused second-level form (MCCONV_FFT2_WORK)
    unsigned* d_cticket = nullptr;  // view, the last word of d_cflag: ticket counter of the riding prefix-sum workgroups (see CorrArgs)
    DevArray<unsigned> d_cflag;     // [ceil(Tmax/256)] launch sequence number per published chunk total
    unsigned cticket_base = 0, cflag_seq = 0;
    // Long settled batches as overlap-save segments of 512 x 8192 frames (ossave.hip.h): whole batches on one fp32 engine whose
    // window carries one set of gains, outside the Q8 regime.  Buffers and the spectra of the sounding (IR set, gains) are
    // made by the first batch that takes the form.
    bool os_hold = false;       // set around a batch whose output pointers are mapped HOST memory (mc_process_batch with pinned buffers)
    bool os_on = true;          // MCCONV_OS=0: such batches through the second-level transform as before (measurement)
    int os_min_blocks = 12288;  // shortest batch that takes the form (a segment costs the same however little of it is used; MCCONV_OS_MIN)
    DevArray<float4> d_os_T;     // [segments][256 row pairs][8192] {row k1, row 512 - k1} between the passes
    DevArray<float4> d_os_part;  // [segments][512 tiles][512] the tiles' sixteenths of the blocks' sums {S1, S2, A1, A2}
    DevArray<float4> d_os_SP, d_os_SP0;  // spectra A, B of the cached key, in the row pass's order
    DevArray<float> d_os_planes;  // gain-weighted taps, four planes
    struct OsKey {
        bool valid = false;
        int n = 0;
        int ir0[MC_MAXV], ir1[MC_MAXV];
        float g[MC_MAXV][4];
        uint64_t gen = 0;
    } os_key;
    uint64_t ir_gen = 0;                  // counts changes of any IR's taps (load, reload, merge)
    uint64_t n_os[2] = {0, 0};            // batches that took the form, spectra builds (mc_debug_read item 11)
    // the small launches of such a batch - prefix sums, the tail's delay-line slots, the last block's segment - run on a side
    // stream beside the three passes, made by the first such batch
    std::unique_ptr<OsSide> os_side;
    int ffa_levels = 3;   // resident MAC in fast-FIR form (up to this many nested levels) when batch and IR are long enough
    bool sliced = false;  // block-sliced calls keep no wet / segment history outside their slices
    int slice_first = -1;  // ... and transform only what their windows reach: the slice start must not move
    bool uniform_valid[2] = {false, false};
    BlockParams uniform_bp[2];

    // avgRuntime (conv.cu:454-462): first 10 calls discarded
    double runtime_ms = 0;
    int nruns = -10;

    // kernel timing
    bool ktiming = false;
    std::unique_ptr<KernelTiming> kt;  // made by the first mc_enable_kernel_timing(on)
    uint32_t kev_blocks[kEvPool];
    bool kev_stamped[kEvPool];            // the launch carries in-kernel time stamps (a single period's sweep)
    int kev_n = 0;  // (KernelTiming::d_stamps: [kStampSlots][MC_STAMP_WGS][2] {start, end} per workgroup in 100 MHz ticks)
    mc_kernel_stats ks;
};

namespace {

size_t y_capacity(const mc_engine* e) { return std::max<size_t>(27 * ((size_t)e->Tcap / 8 + 256) + 1024, 8192); }  // blocks per bin

void host_twiddles(std::vector<float2>& tw) {
    tw.resize(FFT_N);
    for (int m = 0; m < FFT_N; m++) {
        double a = -2.0 * M_PI * (double)m / (double)FFT_N;
        tw[m] = make_float2((float)cos(a), (float)sin(a));
    }
}

void ring_bell(mc_engine* e, unsigned seq, unsigned command) {
    // the period was written before: release order makes it visible to the tail that acquires the doorbell
    if (e->bar_io) {
        _mm_sfence();  // the period's write-combined stores leave before the doorbell's
        __atomic_store_n(reinterpret_cast<unsigned long long*>(e->d_bar.get()), ((unsigned long long)command << 32) | seq, __ATOMIC_RELEASE);
        _mm_sfence();  // ... and the doorbell does not wait in the write-combining buffer
        return;
    }
    __atomic_store_n(e->h_bell, ((unsigned long long)command << 32) | seq, __ATOMIC_RELEASE);
}

// JACK path: a period launched ahead is parked on the engine's stream (process_one).  Before anything else may use the
// stream, or change what the parked tail has already loaded, it is told to give up.  It has written nothing; the next
// mc_process launches that period again.
void unpark(mc_engine* e) {
    // (the cut terms a parked launch summed for the period after its own belong to that launch: without it - told to give up,
    // or timed out and launched again, which rewrites the same buffer with ANOTHER block's terms - they are not to be trusted)
    e->dspec.valid = false;
    if (e->pre.valid) {
        ring_bell(e, e->pre.seq, 1);
        e->pre.valid = false;
        e->n_park_cancel++;
    }
}

hipError_t reset_stamps(mc_engine* e) {
    return hipMemset(e->kt->d_stamps, 0, sizeof(unsigned long long) * e->kt->d_stamps.size());
}

int drain_kernel_events(mc_engine* e) {
    if (!e->kev_n) return MC_OK;
    unpark(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    std::vector<unsigned long long> stamps;
    bool any_stamped = false;
    for (int i = 0; i < e->kev_n; i++) any_stamped = any_stamped || e->kev_stamped[i];
    if (any_stamped) {
        stamps.resize((size_t)2 * MC_STAMP_WGS * kStampSlots);
        HIP_TRY(hipMemcpy(stamps.data(), e->kt->d_stamps, sizeof(unsigned long long) * stamps.size(), hipMemcpyDeviceToHost));
        HIP_TRY(reset_stamps(e));
    }
    for (int i = 0; i < e->kev_n; i++) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->kt->ev[i][0], e->kt->ev[i][1]));
        if (e->kev_stamped[i] && !stamps.empty() && i < kStampSlots) {
            unsigned long long lo = ~0ull, hi = 0;
            const unsigned long long* sp = stamps.data() + (size_t)2 * MC_STAMP_WGS * i;
            for (int w = 0; w < MC_STAMP_WGS; w++)
                if (sp[2 * w]) {
                    lo = std::min(lo, sp[2 * w]);
                    hi = std::max(hi, sp[2 * w + 1]);
                }
            if (hi > lo) ms = (float)((double)(hi - lo) * 1e-5);  // 100 MHz ticks -> ms
        }
        e->kev_stamped[i] = false;
        e->ks.launches++;
        e->ks.blocks += e->kev_blocks[i];
        e->ks.total_ms += ms;
        e->ks.last_ms = ms;
    }
    e->kev_n = 0;
    return MC_OK;
}

// Pipelined mode: nothing of an earlier batch is still running on the post stream
int drain_post(mc_engine* e) {
    if (!e->pipelined) return MC_OK;
    if (e->post_pending[0] || e->post_pending[1]) HIP_TRY(hipStreamSynchronize(e->post_stream));
    e->post_pending[0] = e->post_pending[1] = false;
    return MC_OK;
}

// Pipelined mode: the engine's stream waits for everything issued on the post stream so far
int fence_post(mc_engine* e) {
    if (!e->pipelined) return MC_OK;
    for (int par = 0; par < 2; par++)
        if (e->post_pending[par]) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_post[par], 0));
    return MC_OK;
}

int zero_state(mc_engine* e) {
        unpark(e);
    {
        int rc = drain_post(e);
        if (rc) return rc;
    }
    HIP_TRY(e->d_fdl.zero(e->stream));
    HIP_TRY(e->d_fdl16.zero(e->stream));  // (empty unless precision = fp16)
    HIP_TRY(e->d_slotgain.zero(e->stream));
    HIP_TRY(e->d_seg.zero(e->stream));
    HIP_TRY(e->d_wet.zero(e->stream));
    HIP_TRY(e->d_cring.zero(e->stream));
    HIP_TRY(e->d_xhist.zero(e->stream));
    HIP_TRY(e->d_gring.zero(e->stream));
    HIP_TRY(e->d_res_mac.zero(e->stream));
    HIP_TRY(e->d_res_fix.zero(e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->res_end = e->epoch_b0 = e->cur_delay = 0;
    e->sliced = false;
    e->slice_first = -1;
    for (int i = 0; i < 2; i++)
        for (int v = 0; v < MC_MAXV; v++) e->voice[i][v] = mc_engine::VoiceSlot();
    for (int v = 0; v < MC_MAXV; v++) {
        for (int c = 0; c < 4; c++) e->last_g[v][c] = 0.f;
        e->gain_change_block[v] = 0;
        e->last_nz_voice[v] = 0;
        e->voice_ever[v] = false;
    }
    e->t_abs = e->t_front = 0;
    e->spec_valid = e->dspec.valid = false;
    e->uniform_valid[0] = e->uniform_valid[1] = false;
    e->pipe_head = e->pipe_count = 0;
    return MC_OK;
}

int retire_epoch(mc_engine* e, uint64_t new_delay, bool force);

// An IR's spectra changed (load, reload, mix): everything derived from them - the second-level spectra and the fast-FIR
// components - is rebuilt on next use.  (Round 2 built the fast-FIR components eagerly at every load: 60 MB and three
// launches per 10 s IR for a form that only MCCONV_FFT2=0 selects.)
void invalidate_derived(IrEntry& ir) {
    ir.h2_valid = ir.g2_valid = ir.tail_valid = false;
    ir.hp_valid[0] = ir.hp_valid[1] = ir.hp_valid[2] = false;
}
// The last partitions of an IR's spectra, partition-major, for k_drop_fft: every workgroup of that launch reads the same few
// partitions of all 256 bins, and in the bin-major bank those entries lie Pstride * 16 bytes apart (one 128-byte line fetched per
// 16 bytes used, all of them in one L2 channel).  Worth 2-4 % of the step (round 3, measured with a switch since retired): the launch
// is bound by its latency per workgroup, not by these reads.  kTailSpan partitions cover every predelay the controllers can reach
// (8192 frames = 32 partitions, + 2); a term outside falls back to the bank.
constexpr int kTailSpan = 48;
int ensure_htail(mc_engine* e, const IrEntry* irc) {
    IrEntry& ir = *const_cast<IrEntry*>(irc);
    if (ir.tail_valid || !ir.d_H) return MC_OK;
    if (!ir.d_Htail) HIP_TRY(ir.d_Htail.alloc((size_t)kTailSpan * MC_NB));
    ir.tail_p0 = std::max(0, ir.P - kTailSpan);
    hipLaunchKernelGGL(k_h_tail, dim3(kTailSpan), dim3(MC_NB), 0, e->stream, (const float4*)ir.d_H, e->Pstride, ir.tail_p0, ir.P, ir.d_Htail);
    HIP_TRY(hipGetLastError());
    ir.tail_valid = true;
    return MC_OK;
}
// whether the fast-FIR form of level lvl (1..3) exists for this engine at all
bool hp_possible(const mc_engine* e, int lvl) {
    return !e->half && e->Pstride >= 128 && (e->Pstride >> lvl) >= 32;  // the fp16 MAC streams; small engines never use the fast form
}
// fast-FIR components of an IR's spectra (level lvl) for the resident MAC, built on first use
int ensure_hp(mc_engine* e, hipStream_t st, const IrEntry* irc, int lvl) {
    IrEntry& ir = *const_cast<IrEntry*>(irc);
    if (ir.hp_valid[lvl - 1]) return MC_OK;
    const size_t n = (size_t)(lvl == 1 ? 3 : (lvl == 2 ? 9 : 27)) * MC_NB * (e->Pstride >> lvl);
    if (!ir.d_Hp[lvl - 1]) HIP_TRY(ir.d_Hp[lvl - 1].alloc(n));
    hipLaunchKernelGGL(k_polyphase, dim3(2048), dim3(256), 0, st, ir.d_H, ir.d_Hp[lvl - 1], e->Pstride, lvl);
    HIP_TRY(hipGetLastError());
    ir.hp_valid[lvl - 1] = true;
    return MC_OK;
}

// second-level spectra of an IR (transform of its partition sequence along the block axis), built on first use
int ensure_fft2(mc_engine* e, hipStream_t st, const IrEntry* irc) {
    IrEntry& ir = *const_cast<IrEntry*>(irc);
    if (ir.h2_valid) return MC_OK;
    if (!ir.d_H2) HIP_TRY(ir.d_H2.alloc((size_t)2 * 257 * F2_N));
    // a partition shard transforms its own run of the partition sequence, H[pb .. pe)
    const int pb = std::min<int>((int)e->cfg.part_begin, ir.P), pe = e->cfg.part_end ? std::min<int>((int)e->cfg.part_end, ir.P) : ir.P;
    hipLaunchKernelGGL(k_fft2_ir, dim3(257, 2), dim3(F2_THREADS), 0, st, ir.d_H + pb, e->Pstride, std::min(std::max(pe - pb, 0), F2_N), ir.d_H2);
    HIP_TRY(hipGetLastError());
    ir.h2_valid = true;
    return MC_OK;
}

int ensure_g2(mc_engine* e, hipStream_t st, const IrEntry* irc) {
    IrEntry& ir = *const_cast<IrEntry*>(irc);
    if (ir.g2_valid) return MC_OK;
    if (!ir.d_G2) HIP_TRY(ir.d_G2.alloc((size_t)2 * 257 * G2_N));
    const int pb = std::min<int>((int)e->cfg.part_begin, ir.P), pe = e->cfg.part_end ? std::min<int>((int)e->cfg.part_end, ir.P) : ir.P;
    hipLaunchKernelGGL(k_g2_ir, dim3(257), dim3(G2_THREADS), 0, st, ir.d_H + pb, e->Pstride, std::min(std::max(pe - pb, 0), G2_N), ir.d_G2);
    HIP_TRY(hipGetLastError());
    ir.g2_valid = true;
    return MC_OK;
}

// More IRs are cross-fading in half i than there are voices.  The reference's live spectrum is sum_j c_j H_j and
// every deselected coefficient decays by the same factor per block (f_interpolate, conv.cu:27), so all of the
// half's current IRs - the one being deselected included - merge into ONE spectrum M = sum_j c_j H_j that carries
// on with coefficient 1.  The blocks played so far were weighted IR by IR: everything they still owe is rendered
// into the residual rings first (as for a predelay change), the live pipeline restarts from silence, and the
// half's voices become {M} plus free slots.
int consolidate_voices(mc_engine* e, int i) {
    int rc = retire_epoch(e, e->cur_delay, true);
    if (rc) return rc;
    mc_engine::VoiceSlot* vs = e->voice[i];
    const int buf = 1 - e->mix_buf[i];
    const int midx = kMaxIrs + i * 2 + buf;
    IrEntry& M = e->irs[midx];
    const size_t nH = (size_t)MC_NB * e->Pstride * 4, nh_cap = (size_t)e->cfg.n_ref * 2;
    if (!M.d_H) HIP_TRY(M.d_H.alloc(nH / 4));
    if (!M.d_h) HIP_TRY(M.d_h.alloc(nh_cap / 2));
    MixSrc sH, sh;
    std::memset(&sH, 0, sizeof(sH));
    std::memset(&sh, 0, sizeof(sh));
    double sums[4] = {0, 0, 0, 0}, bound16 = 0.0;
    uint64_t taps = 1;
    int P = 1;
    for (int v = 0; v < MC_MAXV; v++) {
        if (vs[v].ir < 0 || vs[v].coef == 0.0 || !e->irs[vs[v].ir].d_H) continue;
        const IrEntry& src = e->irs[vs[v].ir];
        sH.p[v] = reinterpret_cast<const float*>(src.d_H.get());
        sH.n[v] = nH;
        sH.c[v] = (float)vs[v].coef;
        sh.p[v] = reinterpret_cast<const float*>(src.d_h.get());
        sh.n[v] = (size_t)src.taps * 2;
        sh.c[v] = (float)vs[v].coef;
        for (int c = 0; c < 4; c++) sums[c] += vs[v].coef * src.sums[c];
        taps = std::max(taps, src.taps);
        P = std::max(P, src.P);
        bound16 += std::fabs(vs[v].coef) * 16384.0 / (double)src.scale16;  // |H_j| < 2^14 / scale16_j
    }
    hipLaunchKernelGGL(k_mix, dim3(2048), dim3(256), 0, e->stream, reinterpret_cast<float*>(M.d_H.get()), nH, sH);
    hipLaunchKernelGGL(k_mix, dim3(256), dim3(256), 0, e->stream, reinterpret_cast<float*>(M.d_h.get()), (size_t)taps * 2, sh);
    HIP_TRY(hipGetLastError());
    invalidate_derived(M);
    e->ir_gen++;
    std::memcpy(M.sums, sums, sizeof(sums));
    M.taps = taps;
    M.P = P;
    if (e->half) {
        int ex = 0;
        if (bound16 > 0.0) std::frexp(bound16, &ex);
        M.scale16 = std::ldexp(1.0f, std::min(13 - ex, kScale16MaxExp));
        if (!M.d_H16) HIP_TRY(M.d_H16.alloc(nH / 4));
        hipLaunchKernelGGL(k_to_half, dim3(1024), dim3(256), 0, e->stream, M.d_H, M.d_H16, nH / 4, M.scale16);
        HIP_TRY(hipGetLastError());
    }
    for (int v = 0; v < MC_MAXV; v++) vs[v] = mc_engine::VoiceSlot();
    vs[0].ir = midx;
    vs[0].coef = 1.0;
    e->mix_buf[i] = buf;
    return MC_OK;
}

// voice slot of half i that holds IR `ir`; allocates a free (fully retired) slot when it is new
int voice_slot_for(mc_engine* e, int i, int ir, uint64_t block, int* err) {
    mc_engine::VoiceSlot* vs = e->voice[i];
    for (int v = 0; v < MC_MAXV; v++)
        if (vs[v].ir == ir) return v;
    for (int pass = 0; pass < 2; pass++) {
        // a slot may be reused once its last non-zero gain has left every window (longest IR = Pcap blocks)
        for (int v = 0; v < MC_MAXV; v++)
            if (vs[v].ir < 0 || (vs[v].coef == 0.0 && (!vs[v].ever || vs[v].last_nz + (uint64_t)e->Pcap + 1 < block))) {
                vs[v] = mc_engine::VoiceSlot();
                vs[v].ir = ir;
                return v;
            }
        if (pass == 0) {
            const int rc = consolidate_voices(e, i);
            if (rc) {
                *err = rc;
                return 0;
            }
        }
    }
    *err = fail(MC_ERR_STATE, "no voice slot");
    return 0;
}

// Build the per-block parameter table for T blocks starting at block e->t_front (host, double).
// Advances the cross-fade coefficients exactly like f_interpolate + vsteps-- (conv.cu:27, 339-353).
// Returns pstride (0 = one entry serves all blocks).
int build_params(mc_engine* e, int T, mc_cc_value (&cc)[2], BlockParams** out_tab, int* out_n, int* err) {
    BlockParams* tab = e->h_ptab[e->ptab_next];
    bool all_same = true;
    for (int t = 0; t < T; t++) {
        const uint64_t blk = e->t_front + (uint64_t)t;
        BlockParams& bp = tab[t];
        if (t == 1) {
            // steady state (every cross-fade coefficient has reached its target): the remaining blocks of the batch
            // repeat block 0 - one table entry serves all, whatever the batch length
            bool settled = true;
            for (int i = 0; i < 2; i++) {
                const int sv = voice_slot_for(e, i, (int)cc[i].select, blk, err);
                for (int v = 0; v < MC_MAXV; v++) {
                    const mc_engine::VoiceSlot& s = e->voice[i][v];
                    if (s.ir >= 0 && s.coef != ((v == sv) ? (double)cc[i].wet : 0.0)) settled = false;
                }
            }
            if (settled) {
                const uint64_t last = e->t_front + (uint64_t)T - 1;
                for (int v = 0; v < MC_MAXV; v++) {
                    const float* g = tab[0].g[v];
                    if (g[0] != 0.f || g[1] != 0.f || g[2] != 0.f || g[3] != 0.f) {
                        e->last_nz_voice[v] = last;
                        for (int i = 0; i < 2; i++)
                            if (g[0 * 2 + i] != 0.f || g[1 * 2 + i] != 0.f) e->voice[i][v].last_nz = last;
                    }
                }
                break;
            }
        }
        std::memset(&bp, 0, sizeof(bp));
        // the reference advances its live spectra once per onProcess call: with periods of 512 / 1024 frames the
        // 2 / 4 internal blocks of a call share the call's coefficients
        for (int i = 0; i < 2 && (blk % (uint64_t)e->pm) == 0; i++) {
            const double wet = (double)cc[i].wet;
            const double div = (double)(cc[i].vsteps + 5);
            const int sv = voice_slot_for(e, i, (int)cc[i].select, blk, err);
            if (*err) return 0;
            for (int v = 0; v < MC_MAXV; v++) {
                mc_engine::VoiceSlot& s = e->voice[i][v];
                if (s.ir < 0) continue;
                const double target = (v == sv) ? wet : 0.0;
                s.coef += (target - s.coef) / div;
                // settle: the recurrence converges geometrically; snap once the distance is below double
                // resolution of the reference's float spectra (keeps steady-state tables bit-identical)
                if (std::fabs(target - s.coef) <= 1e-300 + 4e-16 * std::fabs(target) || (target == 0.0 && std::fabs(s.coef) < 1e-14))
                    s.coef = target;
            }
            if (cc[i].vsteps > 0) cc[i].vsteps--;
        }
        for (int i = 0; i < 2; i++) {
            const double lvl = (double)cc[i].level;
            const double pl = pan_l((double)cc[i].panWet), pr = pan_r((double)cc[i].panWet);
            for (int v = 0; v < MC_MAXV; v++) {
                mc_engine::VoiceSlot& s = e->voice[i][v];
                const double c = s.ir >= 0 ? s.coef : 0.0;
                bp.G[v][0 * 2 + i] = pl * lvl * c;
                bp.G[v][1 * 2 + i] = pr * lvl * c;
                bp.g[v][0 * 2 + i] = (float)bp.G[v][0 * 2 + i];
                bp.g[v][1 * 2 + i] = (float)bp.G[v][1 * 2 + i];
                if (bp.g[v][0 * 2 + i] != 0.f || bp.g[v][1 * 2 + i] != 0.f) {
                    s.last_nz = blk;
                    s.ever = true;
                }
            }
            bp.d[0 * 2 + i] = (float)((double)cc[i].dry * pan_l((double)cc[i].panDry) * lvl);
            bp.d[1 * 2 + i] = (float)((double)cc[i].dry * pan_r((double)cc[i].panDry) * lvl);
        }
        for (int v = 0; v < MC_MAXV; v++) {
            if (std::memcmp(e->last_g[v], bp.g[v], sizeof(bp.g[v])) != 0) {
                std::memcpy(e->last_g[v], bp.g[v], sizeof(bp.g[v]));
                e->gain_change_block[v] = blk;
            }
            if (bp.g[v][0] != 0.f || bp.g[v][1] != 0.f || bp.g[v][2] != 0.f || bp.g[v][3] != 0.f) {
                e->last_nz_voice[v] = blk;
                e->voice_ever[v] = true;
            }
        }
        if (t > 0 && std::memcmp(&tab[t], &tab[0], sizeof(BlockParams)) != 0) all_same = false;
    }
    *out_tab = tab;
    *out_n = all_same ? 1 : T;
    return all_same ? 0 : 1;
}

const IrEntry* any_ir(const mc_engine* e) {
    for (int i = 0; i < kMaxIrs; i++)
        if (e->irs[i].d_H) return &e->irs[i];
    return nullptr;
}

// cc[i].value as the call sees it (conv.cu reads the public fields once per onProcess)
int sample_params(mc_engine* e, mc_cc_value (&cc)[2]) {
    e->last_gen = e->ph.sample(cc);
    for (int i = 0; i < 2; i++) {
        if (cc[i].select >= (uint64_t)kMaxIrs || !e->irs[cc[i].select].d_H)
            return fail(MC_ERR_STATE, "half %d selects IR %llu which is not loaded", i, (unsigned long long)cc[i].select);
    }
    if (cc[0].predelay > MC_MAX_PREDELAY) return fail(MC_ERR_ARG, "predelay %llu > %d", (unsigned long long)cc[0].predelay, MC_MAX_PREDELAY);
    return MC_OK;
}

// The voices that can still be heard at block e->t_front, as the MAC sees them
int collect_voices(const mc_engine* e, const BlockParams* first, ActiveVoice* act, int (&vir)[2][MC_MAXV], VoiceSums* vs) {
    if (vs) std::memset(vs, 0, sizeof(*vs));
    const IrEntry* fallback = any_ir(e);
    int nact = 0;
    for (int v = 0; v < MC_MAXV; v++) {
        const IrEntry* ir[2];
        for (int i = 0; i < 2; i++) {
            const int idx = e->voice[i][v].ir;
            vir[i][v] = (idx >= 0 && e->irs[idx].d_H) ? idx : -1;
            ir[i] = vir[i][v] >= 0 ? &e->irs[idx] : nullptr;
            if (ir[i] && vs) {
                for (int c = 0; c < 2; c++) {
                    vs->sig[v][i][c] = ir[i]->sums[c];
                    vs->alp[v][i][c] = ir[i]->sums[2 + c];
                }
            }
        }
        if (!ir[0] && !ir[1]) continue;
        ActiveVoice a;
        a.v = v;
        a.ir0 = ir[0] ? ir[0] : (ir[1] ? ir[1] : fallback);  // a missing half has zero gains; any valid spectra do
        a.ir1 = ir[1] ? ir[1] : a.ir0;
        a.p_end = round_up(std::max(ir[0] ? ir[0]->P : 0, ir[1] ? ir[1]->P : 0), 16);
        // sounding in this batch's windows?  (last non-zero gain not older than the sweep)
        if (!e->voice_ever[v] || e->last_nz_voice[v] + (uint64_t)a.p_end < e->t_front) continue;
        a.uniform = first && e->gain_change_block[v] + (uint64_t)a.p_end <= e->t_front;
        a.ugain = first ? make_float4(first->g[v][0], first->g[v][1], first->g[v][2], first->g[v][3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        act[nact++] = a;
    }
    return nact;
}

int stage_params(mc_engine* e, int T, mc_cc_value (&cc)[2], Staged* st) {
    const int bslot = (int)(e->batch_seq % kPipe);
    BlockParams* d_ptab = e->d_ptab + (size_t)bslot * e->Tmax;

    BlockParams* tab;
    int ntab;
    // reuse of a pinned staging buffer: wait until its previous upload has run
    if (e->ptab_ev_used[e->ptab_next]) HIP_TRY(hipEventSynchronize(e->ptab_ev[e->ptab_next]));
    int berr = MC_OK;
    const uint64_t sampled_vsteps[2] = {cc[0].vsteps, cc[1].vsteps};  // (build_params counts its copy down as it goes)
    const int pstride = build_params(e, T, cc, &tab, &ntab, &berr);
    if (berr) return berr;
    for (int i = 0; i < 2; i++) {
        // vsteps counts down on the engine's copy too (conv.cu:345,353): a compare-exchange against the value this call
        // sampled, so that a select which arrived meanwhile (vsteps = speed, conv.cu:261) is not undone
        const uint64_t used = std::min<uint64_t>(sampled_vsteps[i], (uint64_t)(T / e->pm));
        e->ph.count_down(i, sampled_vsteps[i], used);
        cc[i].vsteps = sampled_vsteps[i] - used;  // (a second staging in the same call - the period parked ahead - goes on from here)
    }
    bool need_upload = true;
    if (pstride == 0 && e->uniform_valid[bslot] && std::memcmp(&e->uniform_bp[bslot], &tab[0], sizeof(BlockParams)) == 0)
        need_upload = false;
    if (need_upload) {
        HIP_TRY(hipMemcpyAsync(d_ptab, tab, sizeof(BlockParams) * (size_t)ntab, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipEventRecord(e->ptab_ev[e->ptab_next], e->stream));
        e->ptab_ev_used[e->ptab_next] = true;
        e->ptab_next = (e->ptab_next + 1) % kStageBufs;
        e->uniform_valid[bslot] = (pstride == 0);
        if (pstride == 0) e->uniform_bp[bslot] = tab[0];
    }
    st->first = tab[0];
    st->d_ptab = d_ptab;
    st->d_sums = e->d_sums + (size_t)bslot * e->Tmax;
    st->ctx.T = T;
    st->ctx.t0 = e->t_front;
    st->ctx.pstride = pstride;
    st->ctx.predelay = cc[0].predelay;
    st->ctx.slot = bslot;
    st->nact = collect_voices(e, &tab[0], st->act, st->ctx.vir, &st->ctx.vs);
    return MC_OK;
}

// Q8 pass descriptor: enabled only when some contribution is shifted past n_ref by the predelay
TailDrop make_taildrop(const mc_engine* e, const int (&vir)[2][MC_MAXV], uint64_t predelay) {
    TailDrop td;
    std::memset(&td, 0, sizeof(td));
    const IrEntry* fb = any_ir(e);
    uint64_t lmax = 0;
    td.nv = MC_MAXV;
    for (int v = 0; v < MC_MAXV; v++) {
        const IrEntry* a = vir[0][v] >= 0 ? &e->irs[vir[0][v]] : nullptr;
        const IrEntry* b = vir[1][v] >= 0 ? &e->irs[vir[1][v]] : nullptr;
        td.h0[v] = a ? a->d_h : (fb ? fb->d_h : nullptr);
        td.h1[v] = b ? b->d_h : (fb ? fb->d_h : nullptr);
        td.L0[v] = a ? (int)a->taps : 0;
        td.L1[v] = b ? (int)b->taps : 0;
        lmax = std::max<uint64_t>(lmax, std::max<uint64_t>(td.L0[v], td.L1[v]));
    }
    td.lmax = (int)lmax;
    // the reference transforms a whole call (pm blocks) at once: its contribution is taps + 256 pm - 1 frames long, and the cut applies to what
    // passes n_ref frames after the START of the call - the last block of a call loses terms (pm - 1) blocks earlier than the first
    // (tests/fuzz/fuzz_q8.py found the condition written for calls of one block: 1024-frame periods with taps + 1023 + predelay > n_ref >= taps + 255 + predelay)
    td.on = (e->cfg.compat && lmax + (uint64_t)(MC_B * e->pm - 1) + predelay > e->cfg.n_ref) ? 1 : 0;
    td.xhist = e->d_xhist;
    td.xr = e->xr;
    td.gring = e->d_gring;
    // the frequency-domain form (k_drop_fft ahead of k_post<3>): fp32 engines whose delay line still holds the blocks the dropped terms come
    // from - up to n_ref / 256 + 2 blocks before the oldest block of the batch (the ring is Tmax + that much or more for every engine that is
    // not created with a batch limit far below its fft size).  MCCONV_TD_FFT=0 (read when the engine is created): the time-domain tiles inside k_post<1> (profiles/r3_shipped_defaults.md
    // has both: 0.40 + 0.21 ms against 0.90 ms per 125 000 blocks at the shipped operating point, 2.5 against 22 ms per step at predelay 8192)
    for (int v = 0; v < MC_MAXV; v++) {
        const IrEntry* a = vir[0][v] >= 0 ? &e->irs[vir[0][v]] : nullptr;
        const IrEntry* b = vir[1][v] >= 0 ? &e->irs[vir[1][v]] : nullptr;
        td.H0s[v] = a ? a->d_H : (fb ? fb->d_H : nullptr);
        td.H1s[v] = b ? b->d_H : (fb ? fb->d_H : nullptr);
        td.P0[v] = a ? a->P : 0;
        td.P1[v] = b ? b->P : 0;
        td.Ht0[v] = a && a->tail_valid ? a->d_Htail : nullptr;
        td.Ht1[v] = b && b->tail_valid ? b->d_Htail : nullptr;
        td.tp0[v] = a && a->tail_valid ? a->tail_p0 : 0;
        td.tp1[v] = b && b->tail_valid ? b->tail_p0 : 0;
    }
    td.pstride_ir = e->Pstride;
    td.fdl = e->d_fdl;
    td.slotgain = e->d_slotgain;
    td.ring = e->ring;
    td.g_tw = e->d_tw;
    td.fft = (e->td_fft && !e->half && (uint64_t)e->ring >= (uint64_t)e->Tmax + e->cfg.n_ref / MC_B + 40) ? 1 : 0;
    return td;
}

// Q8 regime, frequency-domain form (batches): the voices' last partitions partition-major and the buffer of the cut terms, both made by
// the first batch that needs them (on the engine's stream, ahead of k_drop_fft)
int prepare_drop_fft(mc_engine* e, const int (&vir)[2][MC_MAXV], uint64_t predelay) {
    uint64_t lmax = 0;
    for (int h = 0; h < 2; h++)
        for (int v = 0; v < MC_MAXV; v++)
            if (vir[h][v] >= 0) lmax = std::max<uint64_t>(lmax, e->irs[vir[h][v]].taps);
    if (!(e->cfg.compat && lmax + (uint64_t)(MC_B * e->pm - 1) + predelay > e->cfg.n_ref) || e->half || !e->td_fft) return MC_OK;
    for (int h = 0; h < 2; h++)
        for (int v = 0; v < MC_MAXV; v++)
            if (vir[h][v] >= 0) {
                const int rc_t = ensure_htail(e, &e->irs[vir[h][v]]);
                if (rc_t != MC_OK) return rc_t;
            }
    if (!e->d_dropbuf) HIP_TRY(e->d_dropbuf.alloc((size_t)e->Tmax * MC_B));
    return MC_OK;
}

// Whether every output block of a batch (calls of one block) loses exactly ONE (kappa, partition) term, the same for every voice that
// loses anything - then k_fwd<true> sums the cut terms (DropAhead).  The terms of block b: kappa in {0, 1, 2 if predelay % 256},
// partitions p >= n_ref / 256 - predelay / 256 - kappa of every voice's IRs (k_drop_fft).
int plan_drop_ahead(mc_engine* e, const int (&vir)[2][MC_MAXV], uint64_t predelay, DropAhead* da, int* shift) {
    *shift = -1;
    int rc = prepare_drop_fft(e, vir, predelay);
    if (rc != MC_OK) return rc;
    const TailDrop td = make_taildrop(e, vir, predelay);
    if (!td.on || !td.fft || !e->d_dropbuf) return MC_OK;
    const int N = (int)(e->cfg.n_ref / MC_B), a = (int)(predelay >> 8), c = (int)(predelay & 255);
    int kap = -1, part = -1;
    for (int v = 0; v < td.nv; v++) {
        const int pmax = std::max(td.P0[v], td.P1[v]);
        for (int kappa = 0; kappa < (c ? 3 : 2); kappa++)
            for (int p = std::max(N - a - kappa, 0); p < pmax; p++) {
                if (kap >= 0 && (kap != kappa || part != p)) return MC_OK;  // a second term
                kap = kappa, part = p;
            }
    }
    if (kap < 0) return MC_OK;
    for (int v = 0; v < td.nv; v++) {
        da->Ht0[v] = part < td.P0[v] ? (td.Ht0[v] && part >= td.tp0[v] ? td.Ht0[v] + (size_t)(part - td.tp0[v]) * MC_NB : nullptr) : nullptr;
        da->Ht1[v] = part < td.P1[v] ? (td.Ht1[v] && part >= td.tp1[v] ? td.Ht1[v] + (size_t)(part - td.tp1[v]) * MC_NB : nullptr) : nullptr;
        if ((part < td.P0[v] && !da->Ht0[v]) || (part < td.P1[v] && !da->Ht1[v])) return MC_OK;  // (no partition-major copy: k_drop_fft reads the bank)
    }
    da->nv = td.nv;
    da->kappa = kap;
    da->c = c;
    da->shift = kap + a + part;
    da->drop = e->d_dropbuf;
    *shift = da->shift;
    return MC_OK;
}

// JACK path in the Q8 regime: the tail-drop terms of the period that starts at block blk (pm blocks), ahead of its tail kernel
// on the engine's stream (they depend on blocks at least n_ref frames old only).  Returns the buffer the tail reads, or null.
const float* launch_drop_period(mc_engine* e, const TailDrop& td, uint64_t blk, uint64_t predelay) {
    if (!td.on) return nullptr;
    float* dst = e->d_drop[(blk / (uint64_t)e->pm) & 1];
    const int64_t blo = (int64_t)e->epoch_b0;
    if (td.fft) {  // in the frequency domain: a partition sum over the last partitions and one inverse transform per block (k_drop_period_fft)
        if (e->pm == 1)
            hipLaunchKernelGGL(k_drop_period_fft<1>, dim3(1), dim3(64), 0, e->stream, td, dst, (int64_t)blk, (int64_t)predelay, (int64_t)e->cfg.n_ref, blo);
        else if (e->pm == 2)
            hipLaunchKernelGGL(k_drop_period_fft<2>, dim3(1), dim3(128), 0, e->stream, td, dst, (int64_t)blk, (int64_t)predelay, (int64_t)e->cfg.n_ref, blo);
        else
            hipLaunchKernelGGL(k_drop_period_fft<4>, dim3(1), dim3(256), 0, e->stream, td, dst, (int64_t)blk, (int64_t)predelay, (int64_t)e->cfg.n_ref, blo);
        return dst;
    }
    if (e->pm == 1)
        hipLaunchKernelGGL(k_drop_period<1>, dim3(1), dim3(256), 0, e->stream, td, dst, (int64_t)blk, (int64_t)predelay, (int64_t)e->cfg.n_ref, e->rc, blo);
    else if (e->pm == 2)
        hipLaunchKernelGGL(k_drop_period<2>, dim3(1), dim3(256), 0, e->stream, td, dst, (int64_t)blk, (int64_t)predelay, (int64_t)e->cfg.n_ref, e->rc, blo);
    else
        hipLaunchKernelGGL(k_drop_period<4>, dim3(1), dim3(256), 0, e->stream, td, dst, (int64_t)blk, (int64_t)predelay, (int64_t)e->cfg.n_ref, e->rc, blo);
    return dst;
}

// shard of a voice's partition range [p_begin, p_end), multiples of 16
void partition_range(const mc_engine* e, int p_hi, int* p_begin, int* p_end) {
    int pb = (int)e->cfg.part_begin, pe = e->cfg.part_end ? std::min<int>((int)e->cfg.part_end, p_hi) : p_hi;
    if (pb > pe) pb = pe;
    *p_begin = pb;
    *p_end = pe;
}

void launch_mac_stream(mc_engine* e, hipStream_t st, const ActiveVoice& a, int p_lo, int p_hi, int T, int slot0, int nsum, int ch_off,
                       float4* dst = nullptr, unsigned long long* stamps = nullptr) {
    if (!dst) dst = e->d_part;
    const int span = p_hi - p_lo;
    const int chunk = round_up(std::max(1, (span + kNchunk - 1) / kNchunk), 64);
    const dim3 grid(MC_NB, kNchunk, T);
    const float4* sg = e->d_slotgain + (size_t)a.v * e->ring;
    const bool half = e->half && a.ir0->d_H16 && a.ir1->d_H16;
    const void* h0 = half ? (const void*)a.ir0->d_H16 : (const void*)a.ir0->d_H;
    const void* h1 = half ? (const void*)a.ir1->d_H16 : (const void*)a.ir1->d_H;
    const void* fd = half ? (const void*)e->d_fdl16 : (const void*)e->d_fdl;
    const float2 inv = make_float2(1.0f / (a.ir0->scale16 * FDL16_SCALE), 1.0f / (a.ir1->scale16 * FDL16_SCALE));
#define MC_LAUNCH_STREAM(U, H)                                                                                              \
    hipLaunchKernelGGL((k_mac_stream<U, 256, H>), grid, dim3(256), 0, st, h0, h1, e->Pstride, p_lo, p_hi, chunk, fd, sg, \
                       e->ring, slot0, dst, nsum, ch_off, a.ugain, inv, stamps)
    if (a.uniform) {
        if (half) MC_LAUNCH_STREAM(true, true); else MC_LAUNCH_STREAM(true, false);
    } else {
        if (half) MC_LAUNCH_STREAM(false, true); else MC_LAUNCH_STREAM(false, false);
    }
#undef MC_LAUNCH_STREAM
}

// The forms a batch's partition sums take (choose_form and os_applies decide; DESIGN.md §2.5c has the table)
enum class MacForm { Stream, Resident, FastFir, Split, Fused, OverlapSave };

bool second_level(MacForm f) { return f == MacForm::Split || f == MacForm::Fused; }  // the forms that have no 256-block tiles

// mc_kernel_stats.fast_levels of a form: the fast-FIR level 1..3, 0 for the direct forms, 255 / 254 / 253 for the split and the fused
// second-level transform and the overlap-save passes.  Tests and bench.py read these codes.
uint32_t form_code(MacForm f, int level) {
    switch (f) {
        case MacForm::FastFir: return (uint32_t)level;
        case MacForm::Split: return 255u;
        case MacForm::Fused: return 254u;
        case MacForm::OverlapSave: return 253u;
        default: return 0u;
    }
}

// the form's counter in mc_engine::n_mac_form (mc_debug_read item 10), -1: none (the overlap-save passes count in n_os)
int form_counter(MacForm f) {
    switch (f) {
        case MacForm::Fused: return 0;
        case MacForm::Split: return 1;
        case MacForm::FastFir:
        case MacForm::Resident: return 2;
        default: return -1;
    }
}

// Where k_inv finds the partition sums of a batch
struct MacOut {
    MacForm form;
    int lvl;  // fast-FIR levels of the main part (FastFir only)
    const float4* ysrc;
    int64_t sk, stt, sc;
    int nsum;
    int swept;
    int64_t ffa_plane;  // elements between the component sequences (k_inv combines them)
    int main_n;         // blocks described by the fields above; the remaining tail_n blocks of the batch come from
    int tail_n;         // the streaming kernel:
    const float4* tail_ysrc;
    int64_t tail_sk, tail_stt;
    int tail_nsum;
    bool corr_done;  // the Q1/Q2 prefix sums rode along with the launch (k_g2_mac) and are final when it ends

    // n blocks as nsum planes Y[plane][bin][block], sk elements per bin and sc per plane (all forms but the streaming one)
    static MacOut planes(MacForm form, const float4* y, int64_t sk, int nsum, int64_t sc, int n, int swept) {
        MacOut mo = {};
        mo.form = form, mo.ysrc = y, mo.sk = sk, mo.stt = 1, mo.nsum = nsum, mo.sc = sc, mo.main_n = n, mo.swept = swept;
        return mo;
    }
    // n blocks as the streaming kernel leaves them: nsum chunk partials per (block, bin), side by side
    static MacOut partials(const float4* y, int nsum, int n, int swept) {
        MacOut mo = {};
        mo.form = MacForm::Stream, mo.ysrc = y, mo.sk = nsum, mo.stt = (int64_t)MC_NB * nsum, mo.nsum = nsum, mo.sc = 1, mo.main_n = n, mo.swept = swept;
        return mo;
    }
    // ... and the last n blocks of a fast-FIR batch, which come from the streaming kernel
    void add_tail(const float4* y, int nsum, int n) {
        main_n -= n, tail_n = n, tail_ysrc = y, tail_nsum = nsum, tail_sk = nsum, tail_stt = (int64_t)MC_NB * nsum;
    }
};

// inverse transforms of the blocks whose partition sums `mo` describes, into the segment ring from block `b0` -
// or, to_wet, overlap-added straight into the wet ring (only the last block of a launch then stays in the segment ring)
// out != null: the launches also finish the output of their blocks (k_inv_wet<true>, see OutArgs)
void launch_inv(mc_engine* e, const MacOut& mo, uint64_t b0, hipStream_t st, bool to_wet = false, const OutArgs* out = nullptr) {
    auto inv = [&](const float4* y, int64_t sk, int64_t stt, int nsum, int64_t sc, int n, uint64_t b) {
        const int seg0 = (int)(b & (uint64_t)(e->sr - 1));
        if (to_wet) {
            OutArgs oa;
            std::memset(&oa, 0, sizeof(oa));
            if (out) {
                oa = *out;
                oa.blk0 = (int)((int64_t)b - out->tabs0);
            }
            hipLaunchKernelGGL(out ? k_inv_wet<true> : k_inv_wet<false>, dim3((n + IW_NEW - 1) / IW_NEW), dim3(IW_THREADS), 0, st, y, sk, stt, nsum, sc, n,
                               e->d_seg, e->sr, seg0, e->d_wet, e->wr, (int64_t)b * MC_B, e->d_tw, oa);
        } else
            hipLaunchKernelGGL(k_inv, dim3((n + FWD_TILE - 1) / FWD_TILE), dim3(XF_THREADS), 0, st, y, sk, stt, nsum, sc, n, e->d_seg, e->sr,
                               seg0, e->d_tw);
    };
    if (mo.main_n > 0 && mo.form == MacForm::FastFir) {
        const int S = 1 << mo.lvl;
        const dim3 cgrid(((mo.main_n + S - 1) / S + 255) / 256, MC_NB);
        hipLaunchKernelGGL(mo.lvl < 3 ? (mo.lvl == 1 ? k_ffa_combine<1> : k_ffa_combine<2>) : k_ffa_combine<3>, cgrid, dim3(256), 0, st, mo.ysrc,
                           mo.ffa_plane, (int)mo.sk, mo.main_n, e->d_Yc, e->Tcap);
        inv(e->d_Yc, (int64_t)e->Tcap, (int64_t)1, 1, (int64_t)0, mo.main_n, b0);
    } else if (mo.main_n > 0) {
        inv(mo.ysrc, mo.sk, mo.stt, mo.nsum, mo.sc, mo.main_n, b0);
    }
    if (mo.tail_n > 0) inv(mo.tail_ysrc, mo.tail_sk, mo.tail_stt, mo.tail_nsum, (int64_t)1, mo.tail_n, b0 + (uint64_t)mo.main_n);
}

// Taps of the convolution along the block axis that this engine sums: the longest sounding IR's partitions, or the
// engine's shard of them - a shard [pb, pe) is a (pe - pb)-tap convolution whose window starts pb slots earlier.
int block_axis_taps(const mc_engine* e, const ActiveVoice* act, int nact, int* pb_out) {
    int taps = 0, pb0 = (int)e->cfg.part_begin;
    for (int a = 0; a < nact; a++) {
        int pb, pe;
        partition_range(e, act[a].p_end, &pb, &pe);
        taps = std::max(taps, pe - pb);
    }
    if (pb_out) *pb_out = pb0;
    return taps;
}

// What choose_form decides
struct FormChoice {
    MacForm form;
    int lvl;        // FastFir: the levels
    int taps, pb0;  // the second-level forms: the taps of this engine's (shard of the) convolution and where its window starts (block_axis_taps)
    bool per_slot;  // the window does not carry one set of gains: the caller said so, or some voice's gains moved inside it
};

// The form the partition sums of T blocks take, for launch_mac_batch and for run_front, which keeps a sliced window in one launch
// where a second-level form takes it.  (Whether a whole batch goes through the overlap-save passes instead is os_applies' decision,
// further down: it needs the call's pointers and the epoch's state.)
FormChoice choose_form(const mc_engine* e, const ActiveVoice* act, int nact, bool per_slot_gains, int T) {
    FormChoice c = {MacForm::Stream, 0, 0, 0, per_slot_gains};
    for (int a = 0; a < nact; a++) c.per_slot = c.per_slot || !act[a].uniform;
    if (!(T >= e->stream_threshold && !e->half)) return c;
    c.form = MacForm::Resident;
    if (nact <= 0) return c;
    const bool shard = e->cfg.part_begin || e->cfg.part_end;
    c.taps = block_axis_taps(e, act, nact, &c.pb0);
    // both gain layouts are handled (uniform: 2 sequences per bin, fused form; per slot: 4 per voice, split form)
    if (e->fft2 && c.taps <= F2_N / 2) {
        if (!c.per_slot && e->fft2_fused && c.taps <= kG2Pmax) {
            // Uniform gains, fused form: a launch costs ~39 us per chunk of 8192 - taps + 1 blocks whatever the taps; the direct
            // MAC ~10 us + 0.078 ns per block and partition (and never less than ~40 us for the longest IRs: one workgroup
            // sweeps its partitions in turn).  Measured (P = 1728 / 345 / 32): the transform wins from 128 / ~900 / ~9000
            // blocks on - a product of ~300 000 (MCCONV_FFT2_WORK)
            if (c.taps >= 16 && (int64_t)T * c.taps >= e->fft2_work) c.form = MacForm::Fused;
        } else if (T >= 768 && (shard ? c.taps >= 16 && (int64_t)T * c.taps >= 1300000 : c.taps >= 256)) {
            // per-slot gains (or the fused form switched off): the split form, two launches and a stash
            c.form = MacForm::Split;
        }
        if (c.form != MacForm::Resident) return c;
    }
    if (e->ffa_levels > 0 && !shard && hp_possible(e, 1)) {
        int pmin = 1 << 30;
        for (int a = 0; a < nact; a++) pmin = std::min(pmin, act[a].p_end);
        if (e->ffa_levels >= 3 && T >= 8192 && T % 8 == 0 && pmin >= 1024 && hp_possible(e, 3)) c.lvl = 3;
        else if (e->ffa_levels >= 2 && T >= 4096 && T % 4 == 0 && pmin >= 512 && hp_possible(e, 2)) c.lvl = 2;
        else if (T >= 2048 && T % 2 == 0 && pmin >= 256) c.lvl = 1;
        if (c.lvl) c.form = MacForm::FastFir;
    }
    return c;
}

// The voices' second-level spectra (transforms of their partition sequences along the block axis), built on the first batch that
// takes the form: the split form's, or the fused form's
int fft2_voices(mc_engine* e, hipStream_t st, const ActiveVoice* act, int nact, bool fused, Fft2Voices* vv) {
    std::memset(vv, 0, sizeof(*vv));
    for (int a = 0; a < nact; a++) {
        int rc = ensure_fft2(e, st, act[a].ir0);
        if (!rc) rc = ensure_fft2(e, st, act[a].ir1);
        if (!rc && fused) rc = ensure_g2(e, st, act[a].ir0);
        if (!rc && fused) rc = ensure_g2(e, st, act[a].ir1);
        if (rc) return rc;
        vv->h0[a] = fused ? act[a].ir0->d_G2 : act[a].ir0->d_H2;
        vv->h1[a] = fused ? act[a].ir1->d_G2 : act[a].ir1->d_H2;
        vv->g[a] = act[a].ugain;
    }
    vv->n = nact;
    return MC_OK;
}

// Long batches whose window carries one set of gains: the convolution along the block axis as a circular convolution per
// (bin, chunk of blocks) with a second-level transform; the IRs' partition sequences are transformed once.  O(log) instead of
// O(P) work per output block.  Fused form: both inputs' 8192-point spectra side by side in LDS, no stash (k_g2_mac).
// ride != null: the Q1/Q2 prefix sums ride along with the launch (mo->corr_done)
int mac_fused(mc_engine* e, hipStream_t st, const FormChoice& fc, const ActiveVoice* act, int nact, int T, int slot0, const CorrArgs* ride, MacOut* mo) {
    Fft2Voices vv;
    const int rc = fft2_voices(e, st, act, nact, true, &vv);
    if (rc) return rc;
    const int chunk_t = G2_N - fc.taps + 1;
    const int nch = (T + chunk_t - 1) / chunk_t;
    const bool rides = ride && ride->nchunks > 0;
    CorrArgs ca;
    std::memset(&ca, 0, sizeof(ca));
    if (rides) ca = *ride;
    // one workgroup per (bin, chunk) item - the dispatcher keeps two resident per CU and hands a CU its next one the
    // moment a slot frees (measured against 512 persistent workgroups striding over 1280 items: 98 vs 108 us)
    const int main_grid = MC_NB * nch;
    hipLaunchKernelGGL(k_g2_mac, dim3(main_grid + ca.nchunks), dim3(G2B_THREADS), 0, st, e->d_fdl, e->ring, slot0, T, chunk_t, fc.taps, vv,
                       e->d_Yc, e->Tcap, MC_NB * nch, ca, main_grid);
    *mo = MacOut::planes(MacForm::Fused, e->d_Yc, e->Tcap, 1, 0, T, fc.taps);
    mo->corr_done = rides;
    return MC_OK;
}

// Split form of the second-level transform (length F2_N; k_f2_fwd, a stash, k_f2_prod).  One set of gains over the whole window:
// transform the two inputs and weight the products; otherwise transform gain(slot) x input for every voice and path
int mac_split(mc_engine* e, hipStream_t st, const FormChoice& fc, const ActiveVoice* act, int nact, int T, int slot0, MacOut* mo) {
    Fft2Voices vv;
    const int rc = fft2_voices(e, st, act, nact, false, &vv);
    if (rc) return rc;
    const int nseq = fc.per_slot ? 4 * nact : 2;
    Fft2Gains gg;
    std::memset(&gg, 0, sizeof(gg));
    if (fc.per_slot)
        for (int a = 0; a < nact; a++) gg.row[a] = e->d_slotgain + (size_t)act[a].v * e->ring;
    const int chunk_t = F2_N - fc.taps + 1;
    const dim3 grid(MC_NB, (T + chunk_t - 1) / chunk_t);
    const size_t need = (size_t)grid.y * nseq;
    HIP_TRY(e->d_stash.grow(need * MC_NB * F2_N, st));
    hipLaunchKernelGGL(k_f2_fwd, dim3(grid.x * grid.y * nseq), dim3(F2_THREADS), 0, st, e->d_fdl, e->ring, slot0, T, chunk_t, fc.taps, e->d_stash,
                       nseq, gg);
    hipLaunchKernelGGL(k_f2_prod, dim3(grid.x * grid.y * 2), dim3(F2_THREADS), 0, st, e->d_stash, T, chunk_t, fc.taps, vv, e->d_Yc, e->Tcap, nseq);
    *mo = MacOut::planes(MacForm::Split, e->d_Yc, e->Tcap, 1, 0, T, fc.taps);
    return MC_OK;
}

// Fast-FIR form of the convolution along the block axis.  With the polyphase components Xe[n] = X[2n],
// Xo[n] = X[2n+1], He[q] = H[2q], Ho[q] = H[2q+1] (indices relative to the batch start):
//   Y[2n] = (He*Xe)[n] + (Ho*Xo)[n-1],   Y[2n+1] = ((He+Ho)*(Xe+Xo))[n] - (He*Xe)[n] - (Ho*Xo)[n]
// - three convolutions with half the taps and half the outputs: 3/4 of the multiply-adds; applied to each of
// the three again (level 2): nine convolutions at a quarter of the rate, 9/16.  One launch of the resident
// kernel covers all components; k_inv combines them.  Every component is computed for sequence indices
// -1 .. T/2^L - 2, which covers the first T - 2^L blocks of the batch; the last 2^L blocks go through the
// streaming kernel, so that no tile is spent on one extra output.
int mac_fast_fir(mc_engine* e, hipStream_t st, int lvl, const ActiveVoice* act, int nact, bool per_slot_gains, int T, int slot0, MacOut* mo) {
    for (int a = 0; a < nact; a++) {  // the components of this level, built on the first batch that takes it
        int rc = ensure_hp(e, st, act[a].ir0, lvl);
        if (!rc) rc = ensure_hp(e, st, act[a].ir1, lvl);
        if (rc) return rc;
    }
    const int S = 1 << lvl, ncomp = lvl == 1 ? 3 : (lvl == 2 ? 9 : 27);
    const int nh = T / S, ph = e->Pstride >> lvl;
    const int tiles = (nh + 255) / 256;
    const int tcap = tiles * 256;
    const size_t plane = (size_t)MC_NB * tcap;
    const int tail_nsum = nact * kNchunk;  // the last S blocks: streaming kernel, one set of chunk partials per voice
    int swept = 0;
    for (int a = 0; a < nact; a++) {
        const ActiveVoice& av = act[a];
        const int q_end = round_up((av.p_end + S - 1) / S, 16);
        hipLaunchKernelGGL(av.uniform && !per_slot_gains ? k_mac_resident<false> : k_mac_resident<true>, dim3(MC_NB * tiles * ncomp), dim3(256), 0, st,
                           av.ir0->d_Hp[lvl - 1], av.ir1->d_Hp[lvl - 1], ph, 0, q_end, e->d_fdl, e->ring, slot0, nh, av.ugain,
                           e->d_slotgain + (size_t)av.v * e->ring, e->d_Y, tcap, a ? 1 : 0, 1, q_end, lvl, tiles, (int64_t)plane);
        swept = std::max(swept, av.p_end);
    }
    for (int a = 0; a < nact; a++) {
        ActiveVoice av = act[a];
        if (per_slot_gains) av.uniform = false;
        launch_mac_stream(e, st, av, 0, av.p_end, S, (slot0 + T - S) & (e->ring - 1), tail_nsum, a * kNchunk, e->d_tail);
    }
    *mo = MacOut::planes(MacForm::FastFir, e->d_Y, tcap, 1, 0, T, swept);
    mo->lvl = lvl;
    mo->ffa_plane = (int64_t)plane;
    mo->add_tail(e->d_tail, tail_nsum, S);
    return MC_OK;
}

// Resident MAC, direct form, over this engine's (shard of the) partitions
int mac_resident(mc_engine* e, hipStream_t st, const ActiveVoice* act, int nact, bool per_slot_gains, int T, int slot0, MacOut* mo) {
    // short batches: split the partition range so that the launch has ~2048 workgroups
    const int tiles = (T + 255) / 256;
    const int psplit = std::max(1, std::min(8, 8 / tiles));
    const int tcap = psplit > 1 ? tiles * 256 : e->Tcap;  // plane stride of Y (planes summed by k_inv)
    int launched = 0, swept = 0;
    for (int a = 0; a < nact; a++) {
        const ActiveVoice& av = act[a];
        int p_begin, p_end;
        partition_range(e, av.p_end, &p_begin, &p_end);
        if (p_end <= p_begin) continue;
        const int pchunk = round_up((p_end - p_begin + psplit - 1) / psplit, 16);
        hipLaunchKernelGGL(av.uniform && !per_slot_gains ? k_mac_resident<false> : k_mac_resident<true>, dim3(MC_NB * tiles * psplit), dim3(256), 0, st,
                           av.ir0->d_H, av.ir1->d_H, e->Pstride, p_begin, p_end, e->d_fdl, e->ring, slot0, T, av.ugain,
                           e->d_slotgain + (size_t)av.v * e->ring, e->d_Y, tcap, launched ? 1 : 0, psplit, pchunk, 0, tiles, (int64_t)0);
        launched++;
        swept = std::max(swept, p_end - p_begin);
    }
    if (!launched) HIP_TRY(hipMemsetAsync(e->d_Y, 0, sizeof(float4) * (size_t)MC_NB * tcap * psplit, st));
    *mo = MacOut::planes(MacForm::Resident, e->d_Y, tcap, psplit, (int64_t)MC_NB * tcap, T, swept);
    return MC_OK;
}

// streaming MAC: one set of chunk partials per sounding voice, all added by k_inv
int mac_stream(mc_engine* e, hipStream_t st, const ActiveVoice* act, int nact, bool per_slot_gains, int T, int slot0, MacOut* mo) {
    int nv = 0, swept = 0;
    ActiveVoice list[MC_MAXV];
    int pb[MC_MAXV], pe[MC_MAXV];
    for (int a = 0; a < nact; a++) {
        partition_range(e, act[a].p_end, &pb[nv], &pe[nv]);
        if (pe[nv] <= pb[nv]) continue;
        list[nv] = act[a];
        if (per_slot_gains) list[nv].uniform = false;
        nv++;
    }
    const int nsum = std::max(1, nv) * kNchunk;
    if (!nv) HIP_TRY(hipMemsetAsync(e->d_part, 0, sizeof(float4) * (size_t)T * MC_NB * nsum, st));
    for (int a = 0; a < nv; a++) {
        launch_mac_stream(e, st, list[a], pb[a], pe[a], T, slot0, nsum, a * kNchunk);
        swept = std::max(swept, pe[a] - pb[a]);
    }
    *mo = MacOut::partials(e->d_part, nsum, T, swept);
    return MC_OK;
}

// Partition x bin MAC of T blocks starting at delay-line slot `slot0` for the given voices, on stream `st`.
// per_slot_gains: the batch's blocks (or the window) do not share one set of gains.
// ride != null: the Q1/Q2 prefix sums may ride along with the launch (mo->corr_done says whether they did)
int launch_mac_batch(mc_engine* e, hipStream_t st, const ActiveVoice* act, int nact, bool per_slot_gains, int T, int slot0, MacOut* mo,
                     const CorrArgs* ride = nullptr) {
    const FormChoice fc = choose_form(e, act, nact, per_slot_gains, T);
    const int slot2 = (slot0 - fc.pb0) & (e->ring - 1);  // the second-level forms: a shard's window starts pb slots earlier
    int rc;
    switch (fc.form) {
        case MacForm::Fused: rc = mac_fused(e, st, fc, act, nact, T, slot2, ride, mo); break;
        case MacForm::Split: rc = mac_split(e, st, fc, act, nact, T, slot2, mo); break;
        case MacForm::FastFir: rc = mac_fast_fir(e, st, fc.lvl, act, nact, per_slot_gains, T, slot0, mo); break;
        case MacForm::Resident: rc = mac_resident(e, st, act, nact, per_slot_gains, T, slot0, mo); break;
        default: rc = mac_stream(e, st, act, nact, per_slot_gains, T, slot0, mo); break;
    }
    if (!rc && form_counter(fc.form) >= 0) e->n_mac_form[form_counter(fc.form)]++;
    return rc;
}


Retired make_retired(const mc_engine* e) {
    Retired r;
    r.mac = e->d_res_mac;
    r.fix = e->d_res_fix;
    r.rr = e->rr;
    r.end = (int64_t)e->res_end;
    r.b0 = (int64_t)e->epoch_b0;
    return r;
}

int zero_ring_range(mc_engine* e, float* ring, uint64_t from, uint64_t to) {
    // samples [from, to) of a [2][rr] ring indexed by absolute sample; to - from <= rr
    if (to <= from) return MC_OK;
    const uint64_t rr = (uint64_t)e->rr;
    const uint64_t a = from & (rr - 1), n = to - from;
    const uint64_t n1 = std::min(n, rr - a);
    for (int c = 0; c < 2; c++) {
        HIP_TRY(hipMemsetAsync(ring + (size_t)c * rr + a, 0, sizeof(float) * n1, e->stream));
        if (n > n1) HIP_TRY(hipMemsetAsync(ring + (size_t)c * rr, 0, sizeof(float) * (n - n1), e->stream));
    }
    return MC_OK;
}

// K1 over blocks [t_base, t_end) of a batch of T blocks that starts at delay-line slot `slot0` (k_fwd has the parameters' meaning).
// in1 == null: silent blocks into the delay line and nothing else (the inputs are never read); da != null: k_fwd<true>, DropAhead
void launch_fwd(mc_engine* e, hipStream_t st, const float* in1, const float* in2, int T, int slot0, const BlockParams* ptab, int pstride, float4* sums,
                int need_a0, int need_a1, int need_b0, int hist_from, int t_base, int t_end, const DropAhead* da = nullptr, int store_from = 0) {
    const bool live = in1 != nullptr;
    hipLaunchKernelGGL(!da ? k_fwd<false> : k_fwd<true>, dim3((t_end - t_base + FWD_TILE - 1) / FWD_TILE), dim3(XF_THREADS), 0, st, in1, in2, 1,
                       live ? (int64_t)T * MC_B : (int64_t)0, T, e->d_fdl, e->ring, slot0, ptab, pstride, sums, live ? e->d_slotgain : (float4*)nullptr, e->d_tw,
                       e->d_fdl16, live ? e->d_xhist : (float*)nullptr, live ? e->xr : 0, live ? e->d_gring : (float4*)nullptr, live ? e->rc : 0,
                       live ? (int64_t)e->t_front : (int64_t)0, need_a0, need_a1, need_b0, hist_from, t_base, da ? *da : DropAhead(), store_from);
}

// The predelay of the next call differs from the live epoch's.  The reference shifts every call's contribution
// by the predelay current at that call (conv.cu:411-415), so the blocks played so far keep their old offset:
// render what they still owe (partition sums over silent input, Q1/Q2 window terms, Q8 drops) into the
// residual rings and restart the live pipeline from silence under the new predelay.
int retire_epoch(mc_engine* e, uint64_t new_delay, bool force = false) {
    if (new_delay == e->cur_delay && !force) return MC_OK;
    if (e->t_front == e->epoch_b0) {  // nothing has been played under the old value
        e->cur_delay = new_delay;
        return MC_OK;
    }
    if (e->pipe_count) return fail(MC_ERR_STATE, "predelay change / voice merge while a batch awaits mc_finish_batch_device");
    if (e->sliced) return fail(MC_ERR_STATE, "predelay change / voice merge on a block-sliced engine (mc_reset first)");
    {
        int rc = drain_post(e);  // the rings below are rewritten
        if (!rc) unpark(e);
        if (rc) return rc;
    }
    const uint64_t b0 = e->t_front, bs = e->epoch_b0, d_old = e->cur_delay;
    // the latest old call started at block b0 - pm; the reference cuts its contribution n_ref samples later
    const uint64_t new_end = (b0 - (uint64_t)e->pm) * MC_B + e->cfg.n_ref;
    const uint64_t pending_from = std::max<uint64_t>(e->res_end, b0 * MC_B);
    int rc = zero_ring_range(e, e->d_res_mac, pending_from, new_end);
    if (!rc) rc = zero_ring_range(e, e->d_res_fix, pending_from, new_end);
    if (rc) return rc;

    ActiveVoice act[MC_MAXV];
    int vir[2][MC_MAXV];
    const int nact = collect_voices(e, nullptr, act, vir, nullptr);
    int F = 0;  // blocks over which the old blocks still ring: the longest sounding IR
    for (int a = 0; a < nact; a++) F = std::max(F, act[a].p_end);
    // nothing beyond the cut is kept
    F = (int)std::min<uint64_t>((uint64_t)F, (new_end - b0 * MC_B + MC_B - 1) / MC_B);
    if (d_old)
        hipLaunchKernelGGL(k_flush_ring, dim3((unsigned)((d_old + 255) / 256)), dim3(256), 0, e->stream, e->d_wet, e->wr,
                           (int64_t)(b0 * MC_B), (int64_t)d_old, e->d_res_mac, e->rr, (int64_t)new_end);
    uint64_t tv = b0;
    while (F > 0) {
        int Tc = std::min(F, e->Tcap);
        if (!(Tc >= e->stream_threshold && !e->half)) Tc = std::min(Tc, e->Tstream);
        const int slot0 = (int)(tv & (uint64_t)(e->ring - 1));
        launch_fwd(e, e->stream, nullptr, nullptr, Tc, slot0, nullptr, 0, nullptr, 0, Tc, Tc, 0, 0, Tc);  // silent blocks into the delay line
        MacOut mo;
        rc = launch_mac_batch(e, e->stream, act, nact, true, Tc, slot0, &mo);
        if (rc) return rc;
        launch_inv(e, mo, tv, e->stream);
        hipLaunchKernelGGL(k_flush_ola, dim3(Tc), dim3(256), 0, e->stream, e->d_seg, e->sr, (int64_t)tv, (int64_t)d_old,
                           e->d_res_mac, e->rr, (int64_t)new_end);
        tv += (uint64_t)Tc;
        F -= Tc;
    }
    {
        const uint64_t n = new_end - b0 * MC_B;
        hipLaunchKernelGGL(k_flush_fix, dim3((unsigned)((n + MC_B - 1) / MC_B)), dim3(256), 0, e->stream, e->d_cring, e->rc,
                           e->d_res_fix, e->rr, (int64_t)(b0 * MC_B), (int64_t)new_end, (int64_t)bs, (int64_t)b0 - 1, (int64_t)d_old,
                           (int64_t)e->cfg.n_ref, (int)e->cfg.compat, make_taildrop(e, vir, d_old), e->pm);
    }
    HIP_TRY(hipGetLastError());
    // the live pipeline restarts from silence: the old blocks are accounted for
    HIP_TRY(hipMemsetAsync(e->d_fdl, 0, sizeof(float4) * (size_t)MC_NB * e->ring, e->stream));
    if (e->d_fdl16) HIP_TRY(hipMemsetAsync(e->d_fdl16, 0, sizeof(uint2) * (size_t)MC_NB * e->ring, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_seg, 0, sizeof(float) * (size_t)e->sr * 2 * FFT_N, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_wet, 0, sizeof(float) * 2 * (size_t)e->wr, e->stream));
    e->res_end = new_end;
    e->epoch_b0 = b0;
    e->cur_delay = new_delay;
    e->spec_valid = e->dspec.valid = false;
    return MC_OK;
}

// The chunks of 256 blocks the Q1/Q2 prefix sums exist for (CorrArgs): the runs [need_a0, need_a1) and [need_b0, T) of a
// block-sliced rank, everything for a whole batch.  The last block of the batch is always covered (the next call's base).
void corr_chunks(CorrArgs* ca, int T, int need_a0, int need_a1, int need_b0) {
    ca->need_a0 = need_a0;
    ca->need_a1 = need_a1;
    ca->need_b0 = need_b0;
    ca->run0 = need_a0 & ~(CORR_CHUNK - 1);
    ca->nrun0 = need_a1 > ca->run0 ? (std::min(need_a1, T) - ca->run0 + CORR_CHUNK - 1) / CORR_CHUNK : 0;
    const int end0 = ca->run0 + ca->nrun0 * CORR_CHUNK;
    ca->run1 = std::max(std::min(need_b0, T - 1) & ~(CORR_CHUNK - 1), end0);
    const int nrun1 = T > ca->run1 ? (T - ca->run1 + CORR_CHUNK - 1) / CORR_CHUNK : 0;
    ca->nchunks = ca->nrun0 + nrun1;
}

// Arguments of the Q1/Q2 prefix sums of the batch `ctx` describes: its block sums and its parameter table lie in its slot
CorrArgs corr_args(const mc_engine* e, const BatchCtx& ctx) {
    CorrArgs ca;
    std::memset(&ca, 0, sizeof(ca));
    ca.sums = e->d_sums + (size_t)ctx.slot * e->Tmax;
    ca.ptab = e->d_ptab + (size_t)ctx.slot * e->Tmax;
    ca.pstride = ctx.pstride;
    ca.T = ctx.T;
    ca.vs = ctx.vs;
    ca.inv_n = 1.0 / (double)e->cfg.n_ref;
    ca.compat = (int)e->cfg.compat;
    ca.cring = e->d_cring;
    ca.rc = e->rc;
    ca.tabs0 = (int64_t)ctx.t0;
    ca.ctot = e->d_ctot;
    corr_chunks(&ca, ctx.T, ctx.need_a0, ctx.need_a1, ctx.need_b0);
    return ca;
}

// ... as launches of their own (a single chunk adds its base itself)
void launch_corr(hipStream_t st, const CorrArgs& ca) {
    hipLaunchKernelGGL(k_corr_terms, dim3(ca.nchunks), dim3(CORR_CHUNK), 0, st, ca);
    if (ca.nchunks > 1) hipLaunchKernelGGL(k_corr_fix, dim3(ca.nchunks), dim3(CORR_CHUNK), 0, st, ca);
}

// What the launches that finish output themselves (k_inv_wet<true>, k_os_out) need of the batch `ctx` describes: the slice
// ctx.first / ctx.count of a block-sliced engine, or the whole batch from the first block the predelay does not fill from the
// previous call (out_from = wet_head).  lin and drop are the caller's.
OutArgs out_args(const mc_engine* e, const BatchCtx& ctx, bool slice, const float* d_in1, const float* d_in2, float* d_outL, float* d_outR) {
    OutArgs oa;
    std::memset(&oa, 0, sizeof(oa));
    oa.in1 = d_in1;
    oa.in2 = d_in2;
    oa.outL = d_outL;
    oa.outR = d_outR;
    oa.ptab = e->d_ptab + (size_t)ctx.slot * e->Tmax;
    oa.pstride = ctx.pstride;
    oa.cring = e->d_cring;
    oa.rc = e->rc;
    oa.tabs0 = (int64_t)ctx.t0;
    oa.predelay = (int64_t)ctx.predelay;
    oa.n_ref = (int64_t)e->cfg.n_ref;
    oa.b0 = make_retired(e).b0;
    oa.compat = (int)e->cfg.compat;
    oa.pm = e->pm;
    if (slice) {  // the slice [first, first + count), nothing else; a sliced engine keeps no wet history
        oa.out_from = ctx.first;
        oa.out_end = ctx.first + ctx.count;
        oa.out_blk0 = ctx.first;
        oa.wet_head = 0;
        oa.wet_from = 1 << 30;
    } else {
        oa.out_from = oa.wet_head = (int)std::min<uint64_t>((uint64_t)ctx.T, (ctx.predelay + MC_B - 1) / MC_B);
        oa.out_end = ctx.T;
        oa.out_blk0 = 0;
        oa.wet_from = std::max(0, ctx.T - (MC_MAX_PREDELAY / MC_B + 8));  // what later calls and a predelay change can reach
    }
    return oa;
}

// ---------------------------------------------------------------------------
// Long settled batches as overlap-save segments (ossave.hip.h).
// ---------------------------------------------------------------------------
// Can this whole batch take the form?  One engine finishing its own output, one set of gains over the batch and the
// window before it, no retired predelay epoch ringing out, the segments' history inside the live epoch; in the Q8 regime only
// the shipped shape (every output block loses ONE term of ONE source block: the forward transforms sum the cut terms, q8_ok).
bool os_applies(const mc_engine* e, const Staged& st, int count, bool slice, const float* d_in1, const float* d_in2, const float* d_outL,
                const float* d_outR, bool q8_ok, int* ovl_blocks) {
    if (!e->os_on || e->os_hold || e->pipelined || (e->sliced && !slice)) return false;
    if (e->cfg.part_begin || e->cfg.part_end || !d_outL || !d_outR || count < e->os_min_blocks || st.ctx.pstride != 0 || st.nact <= 0) return false;
    // (mc_config.stream_threshold asks for the literal MAC below it; engines with fp16 storage keep it for the partition sweep of
    // single periods and short batches - the spectra of this form come from the fp32 taps whatever the storage of the sweep)
    if (!e->half && count < e->stream_threshold) return false;
    if ((reinterpret_cast<uintptr_t>(d_in1) | reinterpret_cast<uintptr_t>(d_in2) | reinterpret_cast<uintptr_t>(d_outL) | reinterpret_cast<uintptr_t>(d_outR)) & 15) return false;
    int pmax = 0;
    for (int a = 0; a < st.nact; a++) {
        if (!st.act[a].uniform) return false;
        pmax = std::max(pmax, st.act[a].p_end);
    }
    // a block-sliced engine's first segment also carries the blocks whose Q1/Q2 terms its windows reach (their sums come from the column pass)
    const int ovl = slice ? std::max(pmax, (int)(e->cfg.n_ref / MC_B) + MC_MAX_PREDELAY / MC_B + 2) : pmax;
    if (pmax <= 0 || (int64_t)ovl * MC_B > OS_N / 2) return false;  // (a segment at least half new frames)
    if (e->res_end > e->t_front * MC_B) return false;
    if (e->epoch_b0 != 0 && e->epoch_b0 + (uint64_t)pmax > e->t_front) return false;
    if (!q8_ok) return false;  // (Q8 regime in a shape whose cut terms the forward transforms cannot sum themselves)
    *ovl_blocks = ovl;
    return true;
}

// buffers for nseg segments and the spectra of the batch's (IR set, gains)
int ensure_os(mc_engine* e, const Staged& st, int nseg) {
    const size_t seg_el = (size_t)OS_ITEMS * OS_N2;
    const size_t want = (size_t)std::max(nseg, 2);  // (the spectra are built in two segments' worth of it)
    HIP_TRY(e->d_os_T.grow(seg_el * want, e->stream));
    HIP_TRY(e->d_os_part.grow((size_t)OS_TPS * OS_N1 * (size_t)nseg, e->stream));
    if (!e->os_side) HIP_TRY(make_group(e->os_side));
    if (!e->d_os_SP) HIP_TRY(e->d_os_SP.alloc(seg_el * 2));
    if (!e->d_os_SP0) HIP_TRY(e->d_os_SP0.alloc((size_t)2 * OS_N2));
    mc_engine::OsKey key;
    OsMix mix;
    std::memset(&mix, 0, sizeof(mix));
    key.valid = true;
    key.n = st.nact;
    key.gen = e->ir_gen;
    int64_t lmax = 4;
    for (int a = 0; a < MC_MAXV; a++) {
        key.ir0[a] = key.ir1[a] = -1;
        key.g[a][0] = key.g[a][1] = key.g[a][2] = key.g[a][3] = 0.f;
        if (a >= st.nact) continue;
        const ActiveVoice& av = st.act[a];
        key.ir0[a] = (int)(av.ir0 - e->irs);
        key.ir1[a] = (int)(av.ir1 - e->irs);
        key.g[a][0] = av.ugain.x, key.g[a][1] = av.ugain.y, key.g[a][2] = av.ugain.z, key.g[a][3] = av.ugain.w;
        mix.h0[a] = av.ir0->d_h;
        mix.h1[a] = av.ir1->d_h;
        mix.L0[a] = (int)av.ir0->taps;
        mix.L1[a] = (int)av.ir1->taps;
        mix.g[a] = av.ugain;
        lmax = std::max<int64_t>(lmax, std::max<int64_t>(mix.L0[a], mix.L1[a]));
    }
    mix.n = st.nact;
    const mc_engine::OsKey& k0 = e->os_key;
    if (k0.valid && k0.n == key.n && k0.gen == key.gen && !std::memcmp(k0.ir0, key.ir0, sizeof(key.ir0)) &&
        !std::memcmp(k0.ir1, key.ir1, sizeof(key.ir1)) && !std::memcmp(k0.g, key.g, sizeof(key.g)))
        return MC_OK;
    const int64_t np = (lmax + 3) & ~(int64_t)3;
    HIP_TRY(e->d_os_planes.grow(4 * (size_t)np, e->stream));
    e->os_key.valid = false;
    hipLaunchKernelGGL(k_os_ir_mix, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, e->stream, mix, e->d_os_planes, np);
    OsGeo G;
    G.hop = OS_N;
    G.ovl = 0;
    G.n_in = np;
    G.tau0 = 0;
    G.base = 0;
    G.wet_end = np;
    G.seg0 = 0;
    for (int i = 0; i < 2; i++) {
        float4* buf = e->d_os_T + seg_el * i;
        hipLaunchKernelGGL(k_os_cols, dim3(OS_TPS), dim3(OS_THREADS), 0, e->stream, e->d_os_planes + (size_t)np * 2 * i,
                           e->d_os_planes + (size_t)np * (2 * i + 1), (const float*)nullptr, 0, G, buf, (float4*)nullptr, e->d_tw);
        hipLaunchKernelGGL(k_os_rows_fwd, dim3(OS_ITEMS), dim3(G2_THREADS), 0, e->stream, buf);
    }
    hipLaunchKernelGGL(k_os_ir_combine, dim3(OS_ITEMS), dim3(512), 0, e->stream, e->d_os_T, e->d_os_T + seg_el, e->d_os_SP, e->d_os_SP0,
                       0.5f / (float)OS_N);
    HIP_TRY(hipGetLastError());
    e->os_key = key;
    e->n_os[1]++;
    return MC_OK;
}

// The whole batch (T blocks from e->t_front, already staged in `st`) through the overlap-save passes.  Leaves the engine as
// the partitioned passes would: the last blocks' delay-line slots, slot gains and histories (k_fwd over the batch's tail), the
// Q1/Q2 prefix ring, the wet ring where later calls reach, and the last block's segment (its second half opens the next call).
int run_os(mc_engine* e, const Staged& st, mc_engine::BatchCtx& stored, const float* d_in1, const float* d_in2, float* d_outL, float* d_outR,
           int T, int ovl_blocks, int slot0, bool slice, int first, int count, int halo, const DropAhead* q8_da, int q8_shift) {
    // whole batch: wet frames of blocks [0, T).  Block-sliced: of the slice and the reach-back blocks before it (predelay),
    // the segments' history read from the batch's own buffers in front of the window
    const int w0 = slice ? first - halo : 0, wn = slice ? count + halo : T;
    const int64_t ovl = (int64_t)ovl_blocks * MC_B, hop = (int64_t)OS_N - ovl;
    const int hop_blocks = (int)(hop / MC_B);
    const int nseg = (wn + hop_blocks - 1) / hop_blocks;
    int rc = ensure_os(e, st, nseg);
    if (rc) return rc;
    const BlockParams* d_ptab = st.d_ptab;
    // (on HIP's special stream handles - MC_STREAM_DEFAULT = hipStreamLegacy, hipStreamPerThread - everything runs in line:
    // hipStreamWaitEvent on such a handle faults in this runtime)
    const hipStream_t main = e->stream;
    const hipStream_t side = reinterpret_cast<uintptr_t>(main) > 2 ? (hipStream_t)e->os_side->stream : main;
    // A whole batch of two segments or more outside the Q8 regime: the side stream starts behind the column pass, runs the prefix
    // chain the output pass waits for and only then the state later calls read, beside the row pass (which leaves half a CU's
    // wave slots free; the column pass fills them all).  The Q8 regime and block slices produce what the prefix chain or the
    // output pass reads with k_fwd, so there the side stream starts with the call - and so it does for a single segment, whose
    // row and output passes together (about 40 us) are shorter than the side stream's kernels in a row (about 70).
    const bool after = side != main && !slice && q8_shift < 0 && nseg >= 2;
    if (side != main && !after) {  // the side stream starts where the engine's stream stands
        HIP_TRY(hipEventRecord(e->os_side->ev[0], main));
        HIP_TRY(hipStreamWaitEvent(side, e->os_side->ev[0], 0));
    }
    const int hist_from = (int)std::max<int64_t>(0, (int64_t)T - (int64_t)((e->cfg.n_ref + MC_MAX_PREDELAY) / MC_B + 4));
    // the batch's tail: what any later window, Q8 pass or re-render of a predelay epoch can reach
    const int from = std::max(0, T - std::max(round_up(e->Pcap, 16) + 64, (int)((e->cfg.n_ref + MC_MAX_PREDELAY) / MC_B) + 8)) & ~(FWD_TILE - 1);
    auto state_tail = [&]() {  // delay line, slot gains and histories of the tail, no cut terms
        launch_fwd(e, side, d_in1, d_in2, T, slot0, d_ptab, 0, nullptr, 0, 0, from, hist_from, from, T);
    };
    auto last_segment = [&]() {  // the last block's segment from the delay line
        MacOut mo;
        const uint64_t b = e->t_front + (uint64_t)T - 1;
        const int rc_m = launch_mac_batch(e, side, st.act, st.nact, false, 1, (int)(b & (uint64_t)(e->ring - 1)), &mo);
        if (!rc_m) launch_inv(e, mo, b, side);
        return rc_m;
    };
    if (!slice) {
        // state for later calls: delay line, slot gains, input / gain histories of the last blocks (what any later window,
        // Q8 pass or re-render of a predelay epoch can reach), and the last block's segment as the partitioned passes leave it
        // (its partition sums from the delay line, one inverse transform: its second half opens the next call)
        if (q8_shift >= 0) {
            // Q8 regime at the shipped shape: the forward transforms of ALL blocks sum the cut terms of output block t + shift while
            // X_t is in registers (k_fwd<true>, DropAhead) - delay-line slots still only for the tail; the first `shift` output
            // blocks, whose source lies before the batch, through k_drop_fft from the slots the previous call left
            launch_fwd(e, side, d_in1, d_in2, T, slot0, d_ptab, 0, nullptr, 0, T, T, hist_from, 0, T, q8_da, from);
            const TailDrop tdq = make_taildrop(e, st.ctx.vir, st.ctx.predelay);
            const int nd = std::min(T, q8_shift);
            hipLaunchKernelGGL(k_drop_fft, dim3((nd + DF_WAVES - 1) / DF_WAVES), dim3(64 * DF_WAVES), 0, side, tdq, e->d_dropbuf, (int64_t)st.ctx.t0, 0, nd,
                               (int64_t)st.ctx.predelay, (int64_t)e->cfg.n_ref, e->pm, (int64_t)e->epoch_b0);
            (q8_shift < T ? e->n_drop_ahead : e->n_drop_fft)++;
            stored.drop_done = true;
        } else if (!after)
            state_tail();
        if (!after) {
            rc = last_segment();
            if (rc) return rc;
        }
    } else if (stored.need_b0 < T) {
        // block-sliced: the tail of the batch that the next call's windows reach back to (delay line, histories, block sums), as k_fwd leaves it
        launch_fwd(e, side, d_in1, d_in2, T, slot0, d_ptab, 0, st.d_sums, 0, 0, stored.need_b0, hist_from, stored.need_b0 & ~(FWD_TILE - 1), T);
    }
    OutArgs oa = out_args(e, st.ctx, slice, d_in1, d_in2, d_outL, d_outR);
    oa.drop = (!slice && q8_shift >= 0) ? e->d_dropbuf : nullptr;
    OsGeo G;
    G.hop = hop;
    G.ovl = ovl;
    G.n_in = (int64_t)T * MC_B;
    G.tau0 = (int64_t)e->t_front * MC_B;
    G.base = (int64_t)w0 * MC_B;
    G.wet_end = (int64_t)(w0 + wn) * MC_B;
    G.seg0 = 0;
    if (e->ktiming && e->kev_n == kEvPool) {
        rc = drain_kernel_events(e);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_os_cols, dim3(nseg * OS_TPS), dim3(OS_THREADS), 0, main, d_in1, d_in2, (const float*)e->d_xhist, e->xr, G, e->d_os_T,
                       e->cfg.compat ? e->d_os_part : (float4*)nullptr, e->d_tw);
    if (side != main) {  // (with kernel timing the row pass's opening event serves: one marker fewer on the engine's stream)
        const hipEvent_t cols_done = after && e->ktiming ? e->kt->ev[e->kev_n][0] : e->os_side->ev[1];
        HIP_TRY(hipEventRecord(cols_done, main));
        HIP_TRY(hipStreamWaitEvent(side, cols_done, 0));
    }
    {  // Q1/Q2 prefix sums of the batch from the column pass's partial sums, ahead of the output pass
        CorrArgs ca = corr_args(e, st.ctx);
        ca.parts = e->d_os_part;
        ca.parts_hop = hop_blocks;
        ca.parts_ovl = ovl_blocks;
        ca.parts_t0 = w0;
        ca.parts_end = w0 + wn;
        launch_corr(side, ca);
    }
    if (after && e->cfg.compat && e->pm == 1 && !((st.ctx.predelay | e->cfg.n_ref) & (MC_B - 1))) {
        // all frames of a block share their window: its sums once per block instead of per lane of the output pass
        hipLaunchKernelGGL(k_out_windows, dim3((T + 255) / 256), dim3(256), 0, side, oa, T, e->d_wring);
        oa.wring = e->d_wring;
    }
    if (side != main) HIP_TRY(hipEventRecord(e->os_side->ev[2], side));
    if (after) {  // behind the prefix chain, beside the row pass: what later calls read (k_fwd writes the input history the column pass has read)
        state_tail();
        rc = last_segment();
        if (rc) return rc;
        HIP_TRY(hipEventRecord(e->os_side->ev[0], side));
    }
    if (e->ktiming) {
        e->kev_blocks[e->kev_n] = (uint32_t)wn;
        if (!after) HIP_TRY(hipEventRecord(e->kt->ev[e->kev_n][0], main));
    }
    hipLaunchKernelGGL(k_os_rows, dim3(nseg * OS_ITEMS), dim3(G2B_THREADS), 0, main, e->d_os_T, (const float4*)e->d_os_SP, (const float4*)e->d_os_SP0, nseg);
    if (e->ktiming) {
        HIP_TRY(hipEventRecord(e->kt->ev[e->kev_n][1], main));
        e->kev_n++;
        e->ks.resident = 1;
        e->ks.partitions = (uint32_t)ovl_blocks;
        e->ks.fast_levels = form_code(MacForm::OverlapSave, 0);
    }
    if (side != main) HIP_TRY(hipStreamWaitEvent(main, e->os_side->ev[2], 0));  // (the prefix ring and the window sums; where the side stream started with the call, everything it did: the cut terms, and what later calls need)
    hipLaunchKernelGGL(k_os_out, dim3(nseg * OS_TPS), dim3(OS_THREADS), 0, main, (const float4*)e->d_os_T, G, e->d_wet, e->wr, e->d_tw, oa);
    if (after) HIP_TRY(hipStreamWaitEvent(main, e->os_side->ev[0], 0));  // (later calls need the rest of what the side stream did)
    HIP_TRY(hipGetLastError());
    stored.out_from = oa.wet_head;
    stored.corr_done = true;
    e->n_os[0]++;
    return MC_OK;
}

// forward transform + MAC + inverse + overlap-add; lin != null -> sharded partial.
// first/count: the output blocks of the batch this engine will finish (block-sliced operation when count < T):
// everything that later calls depend on (delay line, gains, Q1/Q2 sums, histories) is still produced for all T
// blocks, the partition sums and inverse transforms only for the slice and the few blocks before it that the
// overlap-add and the predelay reach back to.
// d_outL / d_outR != null: the caller finishes the batch right away (run_back follows with the same buffers), so the
// inverse-transform launches may write the output themselves
int run_front(mc_engine* e, const float* d_in1, const float* d_in2, int T, float* lin, int first, int count,
              float* d_outL = nullptr, float* d_outR = nullptr) {
    if (T <= 0 || T > e->Tmax) return fail(MC_ERR_ARG, "nblocks %d outside [1, %d]", T, e->Tmax);
    if (e->pipe_count >= kPipe) return fail(MC_ERR_STATE, "%d batches already await mc_finish_batch_device", kPipe);
    if (T % e->pm) return fail(MC_ERR_ARG, "nblocks %d is not a multiple of the period (%d blocks)", T, e->pm);
        unpark(e);
    const bool slice = !(first == 0 && count == T);
    if (first < 0 || count <= 0 || first + count > T) return fail(MC_ERR_ARG, "slice [%d, %d) outside the batch of %d", first, first + count, T);
    if (slice && lin) return fail(MC_ERR_ARG, "a partition shard cannot be block-sliced");
    if (slice && e->res_end > e->t_front * MC_B) return fail(MC_ERR_STATE, "block-sliced call while a retired predelay epoch is ringing out");
    if (!slice && e->sliced) return fail(MC_ERR_STATE, "whole-batch call on a block-sliced engine (mc_reset first)");
    // pipelined: this batch's parity owns one set of scratch buffers and one slot of the parameter tables; the
    // post stage of the batch two calls ago must be done with them
    const bool piped = e->pipelined && !lin;
    const int par = (int)(e->batch_seq & 1);
    if (e->pipelined && !piped) {
        int rc = drain_post(e);
        if (rc) return rc;
    }
    if (piped) {
        if (e->post_pending[par]) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_post[par], 0));
        e->d_Y = e->d_Ybuf[par];
        e->d_Yc = e->d_Ycbuf[par];
        e->d_part = e->d_partbuf[par];
        e->d_tail = e->d_tailbuf[par];
    }
    const hipStream_t inv_stream = piped ? e->post_stream : e->stream;
    Staged st;
    int halo = 0;  // blocks before the slice that the predelay and the overlap-add reach back to
    {
        mc_cc_value cc[2];
        int rc = sample_params(e, cc);
        if (rc) return rc;
        if (slice) {  // checked before any state advances
            halo = (int)((cc[0].predelay + MC_B - 1) / MC_B) + 1;
            halo = (int)std::min<uint64_t>((uint64_t)halo, e->t_front + (uint64_t)first);  // the stream starts at block 0
            if (count + halo > e->Tcap) return fail(MC_ERR_ARG, "slice of %d blocks + %d blocks of reach-back exceeds the capacity of %d", count, halo, e->Tcap);
            if (e->sliced && e->slice_first != first) return fail(MC_ERR_STATE, "the slice start moved from block %d to %d (mc_reset first)", e->slice_first, first);
        }
        rc = retire_epoch(e, cc[0].predelay);
        if (!rc) rc = stage_params(e, T, cc, &st);
        if (rc) return rc;
    }
    if (slice) {
        e->sliced = true;
        e->slice_first = first;
    }
    // Blocks of this batch that some window of this engine can reach - now (its slice and what lies within one
    // reference length + the largest predelay before it) or from the next call (the same distance before the next
    // slice start).  Only those are transformed; a whole-batch call needs them all.
    int need_a0 = 0, need_a1 = T, need_b0 = T;
    if (slice) {
        const int64_t reach = (int64_t)(e->cfg.n_ref / MC_B) + MC_MAX_PREDELAY / MC_B + 2;
        need_a0 = (int)std::max<int64_t>(0, (int64_t)first - reach);
        need_a1 = first + count;
        need_b0 = (int)std::max<int64_t>(0, std::min<int64_t>(T, (int64_t)T + first - reach));
    }
    const uint64_t wblock = e->t_front + (uint64_t)first - (uint64_t)halo;  // first block of the window (absolute)
    st.ctx.first = first;
    st.ctx.count = count;
    st.ctx.need_a0 = need_a0;
    st.ctx.need_a1 = need_a1;
    st.ctx.need_b0 = need_b0;
    st.ctx.win0 = wblock * MC_B;
    // the finished output comes from this engine alone: overlap-add in the inverse-transform kernel, straight into the
    // wet ring (a partition shard's partial goes through k_ola and the segment ring instead)
    // ... unless the inverse transforms can emit the delayed partial themselves: no retired epoch ringing out)
    const bool lin_fused = lin && e->res_end <= e->t_front * MC_B;
    const bool to_wet = !lin || lin_fused;
    st.ctx.wet_ready = to_wet;
    e->pipe[(e->pipe_head + e->pipe_count) % kPipe] = st.ctx;
    e->spec_valid = e->dspec.valid = false;
    BlockParams* d_ptab = st.d_ptab;
    float4* d_sums = st.d_sums;
    const int pstride = st.ctx.pstride;

    const int slot0 = (int)(e->t_front & (uint64_t)(e->ring - 1));

    {  // long settled batches: overlap-save segments instead of the three passes below (ossave.hip.h)
        int os_ovl = 0;
        const int halo_full = (int)((st.ctx.predelay + MC_B - 1) / MC_B) + 1;
        const bool os_shape = !lin && !piped && to_wet && (!slice || halo == halo_full || wblock == 0);
        DropAhead os_da;
        std::memset(&os_da, 0, sizeof(os_da));
        int os_shift = -1;
        bool q8_ok = true;
        if (os_shape && count >= e->os_min_blocks && make_taildrop(e, st.ctx.vir, st.ctx.predelay).on) {
            q8_ok = false;
            if (!slice && e->os_on && e->pm == 1 && e->epoch_b0 <= e->t_front && e->res_end <= e->t_front * MC_B) {
                const int rc_t = plan_drop_ahead(e, st.ctx.vir, st.ctx.predelay, &os_da, &os_shift);
                if (rc_t != MC_OK) return rc_t;
                q8_ok = os_shift >= 0;
            }
        }
        if (os_shape && os_applies(e, st, count, slice, d_in1, d_in2, d_outL, d_outR, q8_ok, &os_ovl)) {
            const int rc = run_os(e, st, e->pipe[(e->pipe_head + e->pipe_count) % kPipe], d_in1, d_in2, d_outL, d_outR, T, os_ovl, slot0, slice, first, count, halo,
                                  &os_da, os_shift);
            if (rc) return rc;
            e->pipe_count++;
            e->batch_seq++;
            e->t_front += (uint64_t)T;
            return MC_OK;
        }
    }

    // K1: the blocks this engine can reach (all T unless block-sliced).  The input history ring serves the Q8 pass of
    // LATER calls (a batch reads its own samples from its input buffers): they look back less than one reference
    // length + the largest predelay, so a long batch keeps only its tail.
    const int hist_from = (int)std::max<int64_t>(0, (int64_t)T - (int64_t)((e->cfg.n_ref + MC_MAX_PREDELAY) / MC_B + 4));
    DropAhead da;
    std::memset(&da, 0, sizeof(da));
    int da_shift = -1;
    {
        // one launch per run of needed blocks (a whole-batch call: one launch over everything)
        int lo[2] = {need_a0 & ~(FWD_TILE - 1), need_b0 & ~(FWD_TILE - 1)}, hi[2] = {need_a1, T};
        if (lo[1] <= hi[0]) hi[0] = T, lo[1] = T;  // the two runs meet
        // Q8 regime, a whole batch whose output blocks each lose ONE term of ONE source block: the forward transforms sum the cut terms
        // themselves (DropAhead; da_shift = -1 otherwise and k_drop_fft sums them all)
        if (!slice && !lin && to_wet && !e->pipelined && e->pm == 1 && first == 0 && count == T &&
            e->res_end <= e->t_front * MC_B && e->epoch_b0 <= e->t_front && hi[0] == T && lo[0] == 0) {
            const int rc_t = plan_drop_ahead(e, st.ctx.vir, st.ctx.predelay, &da, &da_shift);
            if (rc_t != MC_OK) return rc_t;
        }
        for (int r = 0; r < 2; r++)
            if (hi[r] > lo[r])
                launch_fwd(e, e->stream, d_in1, d_in2, T, slot0, d_ptab, pstride, d_sums, need_a0, need_a1, need_b0, hist_from, lo[r], hi[r],
                           da_shift >= 0 ? &da : nullptr);
    }
    if (e->ktiming && e->kev_n == kEvPool) {
        int rc = drain_kernel_events(e);
        if (rc) return rc;
    }
    int lin_head = 0;  // blocks of a shard's partial that k_ola_head fills (fused form)
    {
        // a window that starts before this batch sees the previous batch's gains too
        bool per_slot = pstride != 0;
        if (slice)
            for (int a = 0; a < st.nact; a++)
                if (e->gain_change_block[st.act[a].v] + (uint64_t)st.act[a].p_end + (uint64_t)halo > e->t_front) per_slot = true;
        // K2 + K3.  The reach-back blocks run as their own short launch (for <= 33 blocks the streaming kernel), so
        // that the slice itself fills whole 256-block tiles of the resident kernel - unless the second-level
        // transform takes the batch, which has no tiles: then the window is one launch.
        const bool whole = halo > 0 && second_level(choose_form(e, st.act, st.nact, per_slot, halo + count).form);
        const int parts[2][2] = {{0, whole ? 0 : halo}, {whole ? 0 : halo, whole ? halo + count : count}};
        for (int h = 0; h < 2; h++) {
            const int off = parts[h][0], n = parts[h][1];
            if (n <= 0) continue;
            const uint64_t b = wblock + (uint64_t)off;
            const bool timed = e->ktiming && h == 1;  // the MAC of the blocks this engine finishes: the roofline kernel
            if (timed) {
                e->kev_blocks[e->kev_n] = (uint32_t)n;
                HIP_TRY(hipEventRecord(e->kt->ev[e->kev_n][0], e->stream));
            }
            MacOut mo;
            // the Q1/Q2 prefix sums of the batch ride along with this launch and the inverse transforms' (fused form only;
            // they read nothing but the block sums k_fwd left and are needed first by k_post)
            CorrArgs ca = corr_args(e, st.ctx);
            // (every riding workgroup looks at the totals of all chunks before it: beyond 160 chunks the two launches of
            // run_back are cheaper than that quadratic chain.  A block-sliced rank has few: only the runs it transforms)
            const bool may_ride = h == 1 && !lin && !piped && to_wet && T > CORR_CHUNK && ca.nchunks > 1 && ca.nchunks <= 160;
            if (may_ride) {
                ca.chain = 1;
                ca.ticket = e->d_cticket;
                ca.ticket_base = e->cticket_base;
                ca.flags = e->d_cflag;
                ca.seq = e->cflag_seq + 1;
            }
            int rc = launch_mac_batch(e, e->stream, st.act, st.nact, per_slot, n, (int)(b & (uint64_t)(e->ring - 1)), &mo, may_ride ? &ca : nullptr);
            if (rc) return rc;
            if (mo.corr_done) {  // the riding workgroups took their tickets
                e->cticket_base += (unsigned)ca.nchunks;
                e->cflag_seq++;
            }
            if (timed) {
                HIP_TRY(hipEventRecord(e->kt->ev[e->kev_n][1], e->stream));
                e->kev_n++;
                e->ks.resident = mo.form != MacForm::Stream ? 1 : 0;
                e->ks.partitions = (uint32_t)mo.swept;
                e->ks.fast_levels = form_code(mo.form, mo.lvl);
            }
            if (piped) {  // the inverse transforms wait for this MAC on the post stream; the engine's stream moves on
                HIP_TRY(hipEventRecord(e->ev_mac[par][h], e->stream));
                HIP_TRY(hipStreamWaitEvent(inv_stream, e->ev_mac[par][h], 0));
            }
            {
                mc_engine::BatchCtx& stored = e->pipe[(e->pipe_head + e->pipe_count) % kPipe];
                // The inverse transforms finish the output themselves when nothing but this batch's own wet signal and
                // final prefix sums go into it: a whole batch on one engine, no Q8 pass, no retired epoch ringing out.
                OutArgs oa;
                std::memset(&oa, 0, sizeof(oa));
                // whole batch: the launch covers it all.  Block-sliced: the launch covers the slice and the reach-back blocks
                // before it, from which the slice's first predelay frames come - unless the stream starts inside the reach-back
                const int halo_full = (int)((st.ctx.predelay + MC_B - 1) / MC_B) + 1;
                const bool covers = slice ? (n == halo + count && off == 0 && halo == halo_full) : (off == 0 && n == T);
                // ... and in the Q8 regime when the cut terms come as a buffer (k_drop_fft, whole batches): they depend on the delay line and
                // the gains only, both complete before the partition sums
                TailDrop tdq = make_taildrop(e, st.ctx.vir, st.ctx.predelay);
                const bool drop_buf = tdq.on && tdq.fft && !slice && !lin;
                bool fuse = lin_fused || (h == 1 && d_outL && d_outR && to_wet && !piped && covers &&
                                          e->res_end <= e->t_front * MC_B && (!tdq.on || drop_buf));
                if (fuse && tdq.on && !lin_fused) {
                    const int rc_t = prepare_drop_fft(e, st.ctx.vir, st.ctx.predelay);
                    if (rc_t != MC_OK) return rc_t;
                    tdq = make_taildrop(e, st.ctx.vir, st.ctx.predelay);  // (with the partition-major spectra)
                    const int nd = da_shift >= 0 ? std::min(T, da_shift) : T;  // (the forward transforms summed the blocks from da_shift on)
                    (da_shift >= 0 && da_shift < T ? e->n_drop_ahead : e->n_drop_fft)++;
                    hipLaunchKernelGGL(k_drop_fft, dim3((nd + DF_WAVES - 1) / DF_WAVES), dim3(64 * DF_WAVES), 0, inv_stream, tdq, e->d_dropbuf, (int64_t)st.ctx.t0, 0, nd,
                                       (int64_t)st.ctx.predelay, (int64_t)e->cfg.n_ref, e->pm, (int64_t)e->epoch_b0);
                    stored.drop_done = true;
                }
                if (fuse) {
                    if (!mo.corr_done && !lin) {  // the prefix sums as launches of their own, ahead of their reader
                        ca.chain = 0;
                        launch_corr(inv_stream, ca);
                        mo.corr_done = true;
                    }
                    oa = out_args(e, st.ctx, slice, d_in1, d_in2, d_outL, d_outR);
                    oa.lin = lin;
                    oa.drop = stored.drop_done ? e->d_dropbuf : nullptr;
                    if (!lin) stored.out_from = oa.wet_head;
                    lin_head = oa.wet_head;
                }
                launch_inv(e, mo, b, inv_stream, to_wet, fuse ? &oa : nullptr);
                if (mo.corr_done) stored.corr_done = true;
            }
            if (piped && h == 0 && count < e->stream_threshold) {
                // both parts would use the streaming kernel's partial buffer: the second waits for the first's reader
                HIP_TRY(hipEventRecord(e->ev_mac[par][0], inv_stream));
                HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_mac[par][0], 0));
            }
        }
    }
    if (lin && lin_fused) {
        if (lin_head > 0)  // the frames the predelay fills from the previous call
            hipLaunchKernelGGL(k_ola_head, dim3(lin_head), dim3(256), 0, e->stream, e->d_wet, e->wr, T, (int64_t)e->t_front,
                               (int64_t)st.ctx.predelay, lin);
    } else if (lin)
        hipLaunchKernelGGL(k_ola, dim3(T), dim3(256), 0, e->stream, e->d_seg, e->sr, T, e->d_wet, e->wr, (int64_t)e->t_front,
                           (int64_t)st.ctx.predelay, make_retired(e), lin);
    HIP_TRY(hipGetLastError());
    e->pipe_count++;
    e->batch_seq++;
    e->t_front += (uint64_t)T;
    return MC_OK;
}

// Q1/Q2 prefix sums, predelay, clamp, dry mix of the oldest batch in flight.
// d_outL == null: the caller does not need this engine's output (a non-root rank of a reduce-to-root): the batch is retired
// and only its Q1/Q2 prefix sums are launched (k_corr_terms / k_corr_fix, unless they rode along with the front half) - the
// history in d_cring has no gaps, so the next batch may be finished here (with output, or a run of it) and a retired epoch
// (k_flush_fix) reads the right sums.  No cut terms, no k_post.
// lin_first / lin_count >= 0 (partition shards after a reduce-scatter): lin_sum holds only blocks [lin_first, lin_first +
// lin_count) of the summed partial, [2][lin_count * 256], and only those blocks are finished (into d_outL / d_outR, which
// start at block lin_first); the Q1/Q2 prefix sums still run over the whole batch - every shard keeps that history.
int run_back(mc_engine* e, const float* d_in1, const float* d_in2, const float* lin_sum, float* d_outL, float* d_outR, int T,
             bool publish = false, int lin_first = -1, int lin_count = -1) {  // publish: the buffers are mapped host memory; raise the completion flag
    if (!e->pipe_count) return fail(MC_ERR_STATE, "no batch awaits its second half");
    const mc_engine::BatchCtx ctx = e->pipe[e->pipe_head];
    if (ctx.T != T) return fail(MC_ERR_ARG, "finish of %d blocks but the pending batch has %d", T, ctx.T);
    const bool lin_slice = lin_first >= 0;
    if (lin_slice && (!lin_sum || lin_count <= 0 || lin_first + lin_count > T || lin_first % e->pm || lin_count % e->pm))
        return fail(MC_ERR_ARG, "slice [%d, %d) of the summed partial outside the batch of %d blocks (or not whole periods)", lin_first, lin_first + lin_count, T);
    e->pipe_head = (e->pipe_head + 1) % kPipe;
    e->pipe_count--;
    const BlockParams* d_ptab = e->d_ptab + (size_t)ctx.slot * e->Tmax;
    // Q1/Q2 prefix sums of this batch, with or without output: run_front left the block sums and the parameter table of the
    // whole batch in the slot on every shard
    if (!ctx.corr_done) {  // (on the headline path they rode along with the front half's launches)
        launch_corr(e->stream, corr_args(e, ctx));
        HIP_TRY(hipGetLastError());
    }
    if (d_outL && d_outR) {
        {
            const int rc_t = prepare_drop_fft(e, ctx.vir, ctx.predelay);
            if (rc_t != MC_OK) return rc_t;
        }
        const bool piped = e->pipelined && !lin_sum && !publish;
        hipStream_t ps = e->stream;
        if (piped) {  // k_post follows this batch's inverse transforms on the post stream, after the prefix sums
            HIP_TRY(hipEventRecord(e->ev_corr[ctx.slot], e->stream));
            HIP_TRY(hipStreamWaitEvent(e->post_stream, e->ev_corr[ctx.slot], 0));
            ps = e->post_stream;
        }
        const TailDrop td_ = make_taildrop(e, ctx.vir, ctx.predelay);
        // the front half finished blocks >= out_from itself: only the blocks the predelay fills from the previous batch remain
        const int post_first = lin_slice ? lin_first : ctx.first;
        const int post_count = lin_slice ? lin_count : (ctx.out_from >= 0 ? ctx.out_from : ctx.count);
        TailDrop td = td_;
        if (post_count > 0 && td.on && td.fft && ctx.drop_done) td.dropbuf = e->d_dropbuf;  // (whole batch, indexed from block 0: post_first is 0 then)
        else if (post_count > 0 && td.on && td.fft) {
            e->n_drop_fft++;
            hipLaunchKernelGGL(k_drop_fft, dim3((post_count + DF_WAVES - 1) / DF_WAVES), dim3(64 * DF_WAVES), 0, ps, td, e->d_dropbuf, (int64_t)ctx.t0, post_first,
                               post_count, (int64_t)ctx.predelay, (int64_t)e->cfg.n_ref, e->pm, (int64_t)e->epoch_b0);
            td.dropbuf = e->d_dropbuf;
        }
        if (post_count > 0 && td.on && !td.fft) e->n_drop_tiles++;
        if (post_count > 0)
        hipLaunchKernelGGL(td.on ? (td.fft ? k_post<3> : k_post<1>) : k_post<0>, dim3((post_count + 3) / 4), dim3(256), 0, ps, ctx.wet_ready ? (const float*)nullptr : e->d_seg, e->sr,
                           lin_sum, e->d_wet, e->wr, e->d_cring,
                           e->rc, d_ptab, ctx.pstride, d_in1, d_in2, d_outL, d_outR, T, (int64_t)ctx.t0, post_first, post_count,
                           ctx.wet_ready ? INT64_MAX : (int64_t)ctx.win0, (int64_t)ctx.predelay, (int64_t)e->cfg.n_ref, (int)e->cfg.compat,
                           td, e->pm, make_retired(e), publish ? e->h_flag.dev() : (unsigned*)nullptr,
                           publish ? ++e->flag_seq : 0u, e->d_done_ctr, lin_slice ? (int64_t)lin_count * MC_B : (int64_t)T * MC_B,
                           lin_slice ? lin_first : 0);
        HIP_TRY(hipGetLastError());
        if (piped) {
            HIP_TRY(hipEventRecord(e->ev_post[ctx.slot], e->post_stream));
            e->post_pending[ctx.slot] = true;
        }
    }
    e->t_abs = ctx.t0 + (uint64_t)T;
    return MC_OK;
}


// The cross-fade has converged and nothing is ramping: staging the next block's parameters now or at the next call
// gives the same table entry (what lets a period be launched one call ahead, see process_one)
bool params_steady(const mc_engine* e, const mc_cc_value (&cc)[2]) {
    for (int i = 0; i < 2; i++) {
        if (cc[i].vsteps != 0) return false;
        bool have = false;
        for (int v = 0; v < MC_MAXV; v++) {
            const mc_engine::VoiceSlot& s = e->voice[i][v];
            if (s.ir < 0) continue;
            if (s.ir == (int)cc[i].select) {
                if (s.coef != (double)cc[i].wet) return false;
                have = true;
            } else if (s.coef != 0.0) {
                return false;
            }
        }
        if (!have) return false;
    }
    return true;
}

// ---- The parked-period protocol: what the period calls share (process_one for 256 frames, process_period_fused for 512 and
// 1024, process_period for shards).  A tail kernel launched one call ahead parks on a doorbell; the next call rings it, tells it
// to give up, or finds that it timed out and launches the period again.  Each piece is defined here once; the plans, the sweep's
// destination, the tail launches and the order of the steps are the paths' own and stay in their functions.

bool same_cc(const mc_cc_value& a, const mc_cc_value& b) {  // (field by field: the struct has padding)
    return a.select == b.select && a.predelay == b.predelay && a.speed == b.speed && a.vsteps == b.vsteps && a.dry == b.dry &&
           a.wet == b.wet && a.panDry == b.panDry && a.panWet == b.panWet && a.level == b.level;
}

// A period of `blocks` blocks into and out of the mapped host buffers (k_fwd / the tails read hd_io, the last kernel writes it)
void period_to_mapped(mc_engine* e, const float* in1, const float* in2, int blocks) {
    const size_t bytes = sizeof(float) * (size_t)blocks * MC_B, cap = (size_t)e->Thost * MC_B;
    std::memcpy(e->h_io + 0 * cap, in1, bytes);
    std::memcpy(e->h_io + 1 * cap, in2, bytes);
}
void copy_period_out(const mc_engine* e, float* outL, float* outR, int blocks) {
    const size_t bytes = sizeof(float) * (size_t)blocks * MC_B, cap = (size_t)e->Thost * MC_B;
    std::memcpy(outL, e->h_io + 2 * cap, bytes);
    std::memcpy(outR, e->h_io + 3 * cap, bytes);
}
// The period where a tail launched now reads it: straight into device memory through the BAR (see mc_engine::d_bar), else mapped memory
void copy_period_in(mc_engine* e, const float* in1, const float* in2, int blocks) {
    if (!e->bar_io) return period_to_mapped(e, in1, in2, blocks);
    const size_t bytes = sizeof(float) * (size_t)blocks * MC_B;
    std::memcpy(e->d_bar + 16, in1, bytes);
    std::memcpy(e->d_bar + 16 + 4 * MC_B, in2, bytes);
    _mm_sfence();  // (write-combined stores: out of the buffers before a doorbell or a launch can refer to them)
}

// The sweep speculation: the sweep of block `blk` is summed in the shadow of the period before it, for the voices the plan of
// that moment sweeps; the call that brings `blk` uses it if its own plan sweeps the same IR pairs (`vir`: the staged block's)
void remember_sweep(mc_engine* e, const ActiveVoice* sweep, int nsweep, const int (&vir)[2][MC_MAXV], uint64_t blk) {
    e->spec_valid = true;
    e->spec_block = blk;
    e->spec_nact = nsweep;
    for (int a = 0; a < nsweep; a++) {
        e->spec_vir[0][a] = vir[0][sweep[a].v];
        e->spec_vir[1][a] = vir[1][sweep[a].v];
    }
}
bool sweep_matches(const mc_engine* e, const ActiveVoice* sweep, int nsweep, const int (&vir)[2][MC_MAXV], uint64_t blk) {
    bool ok = e->spec_valid && e->spec_block == blk && e->spec_nact == nsweep;
    for (int a = 0; a < nsweep && ok; a++) ok = e->spec_vir[0][a] == vir[0][sweep[a].v] && e->spec_vir[1][a] == vir[1][sweep[a].v];
    return ok;
}

// A period's sweep between two events and with in-kernel time stamps when kernel timing is on (the kernel the latency-mode
// roofline is quoted on).  `launch(stamps)` makes the path's launches and returns the span of partitions they swept.
template <class Launch>
int stamped_sweep(mc_engine* e, int blocks, Launch&& launch) {
    const bool timed = e->ktiming;
    if (timed) {
        if (e->kev_n >= kStampSlots) {
            int rc = drain_kernel_events(e);
            if (rc) return rc;
        }
        e->kev_blocks[e->kev_n] = (uint32_t)blocks;
        e->kev_stamped[e->kev_n] = true;
        HIP_TRY(hipEventRecord(e->kt->ev[e->kev_n][0], e->stream));
    }
    const int swept = launch(timed ? e->kt->d_stamps + (size_t)2 * MC_STAMP_WGS * e->kev_n : nullptr);
    if (timed) {
        HIP_TRY(hipEventRecord(e->kt->ev[e->kev_n][1], e->stream));
        e->kev_n++;
        e->ks.resident = 0;
        e->ks.partitions = (uint32_t)swept;
    }
    return MC_OK;
}

// This call's period of `pm` blocks was parked one call ahead, staged with the parameters this call sampled
bool parked_hit(const mc_engine* e, const mc_cc_value (&cc)[2], int pm) {
    return e->pre.valid && e->pre.pm == pm && e->pre.block == e->t_front && same_cc(cc[0], e->pre.cc[0]) && same_cc(cc[1], e->pre.cc[1]) &&
           cc[0].predelay == e->cur_delay;
}
// The next period may be parked: the engine's own stream, a host that spins, and nothing moving
bool may_park(const mc_engine* e, const mc_cc_value (&cc)[2]) {
    return e->park && e->stream == e->own_stream && e->spin_wait && !e->pipelined && !e->ktiming && !e->half && params_steady(e, cc) &&
           cc[0].predelay == e->cur_delay;
}
// The period starting at t_front has been launched with doorbell value `seq` (process_one adds what its kernel carries)
void note_parked(mc_engine* e, const mc_cc_value (&cc)[2], int pm, unsigned seq, const Staged& st) {
    e->pre.valid = true;
    e->pre.pm = pm;
    e->pre.block = e->t_front;
    e->pre.seq = seq;
    e->pre.cc[0] = cc[0];
    e->pre.cc[1] = cc[1];
    e->pre.st = st;
    e->pre.carries_sweep = false;
}

// The output of the period is on the host once `arrived()` says so: spin on it (a JACK callback blocks here anyway; the
// reference blocks in cudaEventSynchronize, conv.cu:455); fall back to a stream sync and `all_there()` if it does not arrive
// in time.  Returns 1 when a parked tail says it gave up on its own.
template <class Arrived, class AllThere>
int spin_for_period(mc_engine* e, unsigned seq, Arrived&& arrived, AllThere&& all_there) {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    for (;;) {
        if (arrived()) return MC_OK;
        if (__atomic_load_n(e->h_exited, __ATOMIC_ACQUIRE) == seq) return 1;
        if ((++spins & 0x3ff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(300)) {
            unpark(e);  // (a kernel parked for the NEXT period would hold the stream until its own timeout)
            HIP_TRY(hipStreamSynchronize(e->stream));
            return all_there() ? MC_OK : fail(MC_ERR_HIP, "period did not complete");
        }
        __builtin_ia32_pause();
    }
}

// The period's last kernel publishes its sequence number in a mapped word
int wait_period(mc_engine* e, unsigned seq) {
    if (!e->spin_wait) {
        HIP_TRY(hipEventSynchronize(e->ev_tail));
        return MC_OK;
    }
    auto published = [&] { return __atomic_load_n(e->h_flag.get(), __ATOMIC_ACQUIRE) == seq; };
    return spin_for_period(e, seq, published, published);
}

// Tagged output (mc_engine::tio): the period's 512 output granules carry its sequence number; they are on the host when every
// tag matches.  Same return values as wait_period.
int wait_period_tagged(mc_engine* e, unsigned seq) {
    const int ngran = 2 * MC_B;
    auto tagged = [&](int i) { return (unsigned)(__atomic_load_n(e->h_gran + i, __ATOMIC_ACQUIRE) >> 32) == seq; };
    auto count_tagged = [&] {
        int i = 0;
        while (i < ngran && tagged(i)) i++;
        return i;
    };
    int first_missing = ngran - 1;  // (stores mostly arrive in order: watch the last one, then check them all)
    auto arrived = [&] {
        while (tagged(first_missing)) {
            const int i = count_tagged();
            if (i == ngran) return true;
            first_missing = i;
        }
        return false;
    };
    return spin_for_period(e, seq, arrived, [&] { return count_tagged() == ngran; });
}

// The end of a period call: wait for period `seq`; when its parked tail gave up on its own (the host was away for more than
// park_ms) the same period is launched the ordinary way, once, behind whatever is queued.  `relaunch(&seq)` is the path's own
// step - unpark, copy, sweep and tail launch in the path's order - and leaves the new sequence number.
template <class Relaunch>
int await_period(mc_engine* e, int (*wait)(mc_engine*, unsigned), unsigned seq, bool relaunch_ok, Relaunch&& relaunch) {
    for (;;) {
        int rc = wait(e, seq);
        if (rc == MC_OK) return MC_OK;
        if (rc != 1) return rc;
        if (!relaunch_ok) return fail(MC_ERR_HIP, "period did not complete");
        relaunch_ok = false;
        e->n_park_timeout++;
        rc = relaunch(&seq);
        if (rc) return rc;
    }
}

// The fused tail of a 512 / 1024-frame period (PM blocks): one workgroup, behind the sweep that filled d_part
template <int PM, bool SELF_DROP>
void launch_tailp(mc_engine* e, const Staged& st, const VoiceSet& vset, int nsum, uint64_t blk, unsigned seq, const TailDrop& tdp,
                  const unsigned long long* bell, const float* drop) {
    const size_t cap = (size_t)e->Thost * MC_B;
    const float *pin1 = e->bar_io ? e->d_bar + 16 : e->h_io.dev() + 0 * cap, *pin2 = e->bar_io ? e->d_bar + 16 + 4 * MC_B : e->h_io.dev() + 1 * cap;
    hipLaunchKernelGGL((k_tailp<PM, SELF_DROP>), dim3(1), dim3(256), 0, e->stream, pin1, pin2, vset, e->Pstride, e->d_fdl, e->d_slotgain,
                       e->ring, (int)(blk & (uint64_t)(e->ring - 1)), e->d_part, nsum, st.d_ptab, e->d_seg, e->sr, e->d_wet, e->wr, e->d_cring,
                       e->rc, st.ctx.vs, 1.0 / (double)e->cfg.n_ref, (int)e->cfg.compat, (int64_t)blk, (int64_t)st.ctx.predelay,
                       (int64_t)e->cfg.n_ref, e->h_io.dev() + 2 * cap, e->h_io.dev() + 3 * cap, e->d_tw, tdp, e->d_fdl16, e->h_flag.dev(), seq,
                       make_retired(e), bell, e->hd_exited, e->park_ticks, drop, nullptr, nullptr);
}

// One JACK period with host buffers (Convolution::onProcess, conv.cu:287-466): zero-copy I/O through mapped pinned
// memory, the streaming MAC over the partitions that do not depend on the new block, and the fused k_tail1.
//
// Who sums what.  An engine that owns the IR's first partitions (every engine but a partition shard with
// part_begin > 0): the tail takes partition 0 (the new block) and partition 1 (the previous block, from the delay
// line); the streaming sweep takes partitions >= 2 - they pair with blocks at least two periods old, so the sweep of
// period t + 1 depends on nothing period t produces.  A shard that starts later sweeps its whole range.
//
// Launching a period ahead.  Measured (MC_JACK_TRACE build, profiles/r2_jack_trace.md): of 16 us per back-to-back call
// the tail kernel works 6.5 us; the rest is the host's launch call and the dispatch latency that follow the arrival of
// the period.  So, in the steady state, call t launches - behind the tail of period t - ONE kernel (k_jack) whose
// workgroup 0 is the tail of period t + 1 and whose other workgroups are the sweep of period t + 2.  The tail requests
// everything it needs except the period itself and parks on a doorbell in mapped memory; call t + 1 copies the period
// in, rings, and waits for the completion word: no launch on the critical path.  The parameters a parked period was
// staged with are compared with the ones the next call samples; any difference (a controller moved, an IR was
// selected) tells it to give up - it has written nothing - and the period is launched the ordinary way.  A parked
// tail that hears nothing for 100 ms gives up on its own (a host that stopped calling must not leave a kernel behind).
int process_one(mc_engine* e, const float* in1, const float* in2, float* outL, float* outR) {
    if (!in1 || !in2 || !outL || !outR) return fail(MC_ERR_ARG, "null buffer");
    if (e->pipe_count) return fail(MC_ERR_STATE, "a sharded batch is still pending");
    if (e->sliced) return fail(MC_ERR_STATE, "single-period call on a block-sliced engine (mc_reset first)");
#ifdef MC_JACK_TRACE
    const auto tr0 = std::chrono::steady_clock::now();
#endif
    const size_t cap = (size_t)e->Thost * MC_B;
    mc_cc_value cc[2];
    {
        int rc = sample_params(e, cc);
        if (rc) return rc;
    }

    // ---- the voices and ranges of a staged block
    struct Plan {
        ActiveVoice sweep[MC_MAXV];
        int lo[MC_MAXV], hi[MC_MAXV], nsweep = 0, nsum = 1;
        VoiceSet vset;
    };
    auto make_plan = [&](const Staged& st, Plan& pl) {
        std::memset(&pl.vset, 0, sizeof(pl.vset));
        pl.nsweep = 0;
        for (int a = 0; a < st.nact; a++) {
            int pb, pe;
            partition_range(e, st.act[a].p_end, &pb, &pe);
            if (pe <= pb) continue;
            if (pb == 0) {
                pl.vset.vid[pl.vset.n] = st.act[a].v;
                pl.vset.H0[pl.vset.n] = st.act[a].ir0->d_H;
                pl.vset.H1[pl.vset.n] = st.act[a].ir1->d_H;
                pl.vset.n++;
            }
            const int first = pb == 0 ? 2 : pb;
            if (pe > first) {
                pl.sweep[pl.nsweep] = st.act[a];
                pl.lo[pl.nsweep] = first;
                pl.hi[pl.nsweep] = pe;
                pl.nsweep++;
            }
        }
        pl.nsum = std::max(1, pl.nsweep) * kNchunk;
    };
    auto sweep_uniform = [&](const ActiveVoice& av, int hi, uint64_t blk) {
        // one gain for all slots only when the last change is older than every slot of the sweep
        return e->gain_change_block[av.v] + (uint64_t)hi <= blk && e->gain_change_block[av.v] < blk;
    };
    // standalone sweep of block `blk` into its partial buffer (timed: the kernel the latency-mode roofline is quoted on)
    auto launch_sweep = [&](const Plan& pl, uint64_t blk) -> int {
        float4* dst = e->d_part_jack[blk & 1];
        if (!pl.nsweep) {
            HIP_TRY(hipMemsetAsync(dst, 0, sizeof(float4) * (size_t)MC_NB * pl.nsum, e->stream));
            return MC_OK;
        }
        return stamped_sweep(e, 1, [&](unsigned long long* stamps) {
            const int bslot0 = (int)(blk & (uint64_t)(e->ring - 1));
            int swept = 0;
            for (int a = 0; a < pl.nsweep; a++) {
                ActiveVoice av = pl.sweep[a];
                av.uniform = sweep_uniform(av, pl.hi[a], blk);
                launch_mac_stream(e, e->stream, av, pl.lo[a], pl.hi[a], 1, bslot0, pl.nsum, a * kNchunk, dst, stamps);
                swept = std::max(swept, pl.hi[a] - (pl.lo[a] == 2 ? 0 : pl.lo[a]));
            }
            return swept;
        });
    };
    int prep_rc = MC_OK;  // first failure of prepare_drop_fft inside tail_args (checked behind every launch that used it)
    auto tail_args = [&](const Staged& st, const Plan& pl, uint64_t blk, unsigned seq, bool parked) {
        TailArgs A;
        std::memset(&A, 0, sizeof(A));
        A.in1 = e->bar_io ? e->d_bar + 16 : e->h_io.dev() + 0 * cap;
        A.in2 = e->bar_io ? e->d_bar + 16 + 4 * MC_B : e->h_io.dev() + 1 * cap;
        A.vset = pl.vset;
        A.pstride_ir = e->Pstride;
        A.fdl = e->d_fdl;
        A.slotgain = e->d_slotgain;
        A.ring = e->ring;
        A.slot0 = (int)(blk & (uint64_t)(e->ring - 1));
        A.part = e->d_part_jack[blk & 1];
        A.nsum = pl.nsum;
        A.ptab = st.d_ptab;
        A.seg = e->d_seg;
        A.sr = e->sr;
        A.seg0 = (int)(blk & (uint64_t)(e->sr - 1));
        A.wet = e->d_wet;
        A.wr = e->wr;
        A.cring = e->d_cring;
        A.rc = e->rc;
        A.vs = st.ctx.vs;
        A.inv_n = 1.0 / (double)e->cfg.n_ref;
        A.compat = (int)e->cfg.compat;
        A.tabs0 = (int64_t)blk;
        A.predelay = (int64_t)st.ctx.predelay;
        A.n_ref = (int64_t)e->cfg.n_ref;
        A.outL = e->h_io.dev() + 2 * cap;
        A.outR = e->h_io.dev() + 3 * cap;
        A.g_tw = e->d_tw;
        {  // (Q8 regime: the last partitions partition-major and the buffer of the cut terms)
            const int r = prepare_drop_fft(e, st.ctx.vir, st.ctx.predelay);
            if (r != MC_OK && prep_rc == MC_OK) prep_rc = r;
        }
        A.td = make_taildrop(e, st.ctx.vir, st.ctx.predelay);
        A.fdl16 = e->d_fdl16;
        A.done_flag = e->h_flag.dev();
        A.seq = seq;
        A.ret = make_retired(e);
        A.bell = parked ? (e->bar_io ? reinterpret_cast<unsigned long long*>(e->d_bar.get()) : e->hd_bell) : nullptr;
        A.exited = e->hd_exited;
        A.park_ticks = e->park_ticks;
        {
            const mc_engine::DropSpec& ds = e->dspec;
            if (A.td.on && ds.valid && ds.block == blk && ds.predelay == st.ctx.predelay && ds.epoch_b0 == e->epoch_b0 &&
                std::memcmp(ds.vir, st.ctx.vir, sizeof(ds.vir)) == 0) {
                A.drop = ds.buf;  // (summed by the launch before this one)
                e->n_drop_carried++;
            } else
                A.drop = launch_drop_period(e, A.td, blk, st.ctx.predelay);  // (queued ahead of the tail this argument block is for)
        }
        A.formcount = e->d_tailform;
        A.form = e->tail_form;
        A.in_gran = e->tio ? reinterpret_cast<const unsigned long long*>(reinterpret_cast<const char*>(e->d_bar.get()) + 16384) : nullptr;
        A.out_gran = e->tio ? e->h_gran.dev() : nullptr;
        return A;
    };

    // ---- this period: a parked tail staged with the same parameters, or the ordinary launch
    unsigned my_seq = 0;
    bool relaunch_ok = false;  // (a parked period that gave up on its own can be launched again as it was staged)
    Staged st_now;
    Plan pl_now;
    if (parked_hit(e, cc, 1)) {
        my_seq = e->pre.seq;
        if (e->tio) {
            // tagged input: the period as granules {sample, sequence number} straight into device memory - every lane of the
            // parked tail is polling its own two; no doorbell, no second round trip for the data it would announce
            volatile unsigned long long* g = reinterpret_cast<volatile unsigned long long*>(reinterpret_cast<char*>(e->d_bar.get()) + 16384);
            const unsigned long long tag = (unsigned long long)my_seq << 32;
            for (int i = 0; i < MC_B; i++) {
                uint32_t a, b;
                std::memcpy(&a, in1 + i, 4);
                std::memcpy(&b, in2 + i, 4);
                g[i] = tag | a;
                g[MC_B + i] = tag | b;
            }
            _mm_sfence();
        } else {
            copy_period_in(e, in1, in2, 1);
            ring_bell(e, my_seq, 0);
        }
        e->pre.valid = false;
        e->n_park_hit++;
        st_now = e->pre.st;
        pl_now = Plan();
        make_plan(st_now, pl_now);
        relaunch_ok = true;
        // the sweep the parked kernel carries is the one the NEXT period will use
        e->spec_valid = false;
        if (e->pre.carries_sweep) {
            e->spec_valid = true;
            e->spec_block = e->t_front + 1;
            e->spec_nact = 1;
            e->spec_vir[0][0] = e->pre.carried_vir[0];
            e->spec_vir[1][0] = e->pre.carried_vir[1];
        }
    } else {
        unpark(e);
        copy_period_in(e, in1, in2, 1);
        {
            int rc = drain_post(e);
            if (!rc) rc = retire_epoch(e, cc[0].predelay);
            if (!rc) rc = stage_params(e, 1, cc, &st_now);
            if (rc) return rc;
        }
        make_plan(st_now, pl_now);
        if (!sweep_matches(e, pl_now.sweep, pl_now.nsweep, st_now.ctx.vir, e->t_front)) {
            int rc = launch_sweep(pl_now, e->t_front);
            if (rc) return rc;
        }
        e->spec_valid = false;
        my_seq = ++e->flag_seq;
        hipLaunchKernelGGL(k_tail1, dim3(1), dim3(TAIL1_THREADS), 0, e->stream, tail_args(st_now, pl_now, e->t_front, my_seq, false));
        if (prep_rc) return prep_rc;
        HIP_TRY(hipGetLastError());
    }
    if (!e->spin_wait) HIP_TRY(hipEventRecord(e->ev_tail, e->stream));
    e->batch_seq++;
    e->t_front += 1;
    e->t_abs = e->t_front;

    // ---- the next period: parked one call ahead when nothing is moving, else only its sweep (as a speculation: every
    // slot carries its own gains, so it stays exact under any parameter change except a change of the sounding IR set
    // or an IR reload, which the next call checks)
    bool parked_next = false;
    if (may_park(e, cc)) {
        Staged st_next;
        int rc = stage_params(e, 1, cc, &st_next);  // (steady: advancing the cross-fade by a block changes nothing)
        if (rc) return rc;
        Plan pl_next;
        make_plan(st_next, pl_next);
        if (st_next.ctx.pstride == 0 && pl_next.nsweep <= 1 && std::memcmp(&st_next.first, &st_now.first, sizeof(BlockParams)) == 0) {
            // the sweep of the period about to be parked, unless the kernel ahead of it already carries it
            if (!sweep_matches(e, pl_next.sweep, pl_next.nsweep, st_next.ctx.vir, e->t_front)) {
                rc = launch_sweep(pl_next, e->t_front);
                if (rc) return rc;
                remember_sweep(e, pl_next.sweep, pl_next.nsweep, st_next.ctx.vir, e->t_front);
            }
            const unsigned seq = ++e->flag_seq;
            TailArgs A = tail_args(st_next, pl_next, e->t_front, seq, true);
            if (prep_rc) return prep_rc;
            SweepArgs S;
            std::memset(&S, 0, sizeof(S));
            const uint64_t blk2 = e->t_front + 1;  // the sweep this kernel carries
            bool uni = true;
            if (pl_next.nsweep == 1) {
                const ActiveVoice& av = pl_next.sweep[0];
                const int span = pl_next.hi[0] - pl_next.lo[0];
                uni = sweep_uniform(av, pl_next.hi[0], blk2);
                S.H0 = av.ir0->d_H;
                S.H1 = av.ir1->d_H;
                S.pstride_ir = e->Pstride;
                S.p_begin = pl_next.lo[0];
                S.p_end = pl_next.hi[0];
                S.chunk = round_up(std::max(1, (span + kNchunk - 1) / kNchunk), 64);
                S.fdl = e->d_fdl;
                S.slotgain = e->d_slotgain + (size_t)av.v * e->ring;
                S.ring = e->ring;
                S.slot0 = (int)(blk2 & (uint64_t)(e->ring - 1));
                S.part = e->d_part_jack[blk2 & 1];
                S.nsum = pl_next.nsum;
                S.ch_off = 0;
                S.ugain = av.ugain;
                S.inv = make_float2(1.f, 1.f);
                S.nchunk = kNchunk;
            }
            // the cut terms of the period after the parked one ride along (its sweep does: same launch, one more workgroup)
            const bool carry = A.td.on && A.td.fft && e->pm == 1;
            S.drop_next = carry ? e->d_drop[blk2 & 1] : nullptr;
            const dim3 grid(1 + (pl_next.nsweep == 1 ? MC_NB * kNchunk : 0) + (carry ? 1 : 0));
            e->dspec.valid = false;
            if (carry) {
                e->dspec.valid = true;
                e->dspec.block = blk2;
                e->dspec.predelay = st_next.ctx.predelay;
                e->dspec.epoch_b0 = e->epoch_b0;
                std::memcpy(e->dspec.vir, st_next.ctx.vir, sizeof(e->dspec.vir));
                e->dspec.buf = S.drop_next;
            }
            if (uni)
                hipLaunchKernelGGL(k_jack<true>, grid, dim3(TAIL1_THREADS), 0, e->stream, A, S);
            else
                hipLaunchKernelGGL(k_jack<false>, grid, dim3(TAIL1_THREADS), 0, e->stream, A, S);
            HIP_TRY(hipGetLastError());
            note_parked(e, cc, 1, seq, st_next);
            e->pre.carries_sweep = pl_next.nsweep == 1;
            if (pl_next.nsweep == 1) {
                e->pre.carried_vir[0] = st_next.ctx.vir[0][pl_next.sweep[0].v];
                e->pre.carried_vir[1] = st_next.ctx.vir[1][pl_next.sweep[0].v];
            }
            parked_next = true;
        }
    }
    if (!parked_next) {
        // (not steady, or more than one voice sounding: the next period's sweep alone, in the shadow of this period)
        Staged& st = st_now;
        Plan& pl = pl_now;
        if (pl.nsweep && !(e->spec_valid && e->spec_block == e->t_front)) {
            int rc = launch_sweep(pl, e->t_front);
            if (rc) return rc;
            remember_sweep(e, pl.sweep, pl.nsweep, st.ctx.vir, e->t_front);
        }
    }
#ifdef MC_JACK_TRACE
    const auto tr1 = std::chrono::steady_clock::now();
#endif
    // the output of THIS block is on the host once its tail has published its sequence number (await_period).  When the
    // parked tail gave up on its own, the same period is launched the ordinary way behind whatever is queued:
    auto relaunch = [&](unsigned* seq) -> int {
        unpark(e);  // (the kernel parked for the period after this one must not run before it)
        copy_period_in(e, in1, in2, 1);  // (a tail launched now reads the plain copy of the period)
        // That kernel (launched above, behind a tail that had already left the stream) ran at once: the sweep it carries - the
        // one of the period after next - went into the partial-sum buffer of THIS period (same parity) and read a delay line
        // without this period's block.  unpark() has forgotten it; this period's own partial sums are summed again, on the
        // same stream behind the stray sweep.
        int rc = launch_sweep(pl_now, e->t_front - 1);
        if (rc) return rc;
        *seq = ++e->flag_seq;
        hipLaunchKernelGGL(k_tail1, dim3(1), dim3(TAIL1_THREADS), 0, e->stream, tail_args(st_now, pl_now, e->t_front - 1, *seq, false));
        if (prep_rc) return prep_rc;
        HIP_TRY(hipGetLastError());
        return MC_OK;
    };
    {
        int rc = await_period(e, e->tio ? wait_period_tagged : wait_period, my_seq, relaunch_ok, relaunch);
        if (rc) return rc;
    }
#ifdef MC_JACK_TRACE
    const auto tr2 = std::chrono::steady_clock::now();
#endif
    if (e->tio) {
        for (int i = 0; i < MC_B; i++) {
            const uint32_t a = (uint32_t)e->h_gran[i], b = (uint32_t)e->h_gran[MC_B + i];
            std::memcpy(outL + i, &a, 4);
            std::memcpy(outR + i, &b, 4);
        }
    } else {
        copy_period_out(e, outL, outR, 1);
    }
#ifdef MC_JACK_TRACE
    {
        const auto tr3 = std::chrono::steady_clock::now();
        const unsigned long long* w = reinterpret_cast<const unsigned long long*>(e->h_flag);
        if (e->tr_n >= 100) {  // (skip the warm-up)
            e->tr_launch += std::chrono::duration<double, std::micro>(tr1 - tr0).count();
            e->tr_flag += std::chrono::duration<double, std::micro>(tr2 - tr0).count();
            e->tr_total += std::chrono::duration<double, std::micro>(tr3 - tr0).count();
            e->tr_kernel += (double)(w[2] - w[1]) * 0.01;
            e->tr_out += (double)(w[3] - w[1]) * 0.01;
            e->tr_clk += (double)w[4];
            for (int i = 0; i < 3; i++) e->tr_c[i] += (double)w[5 + i];
            if (e->tr_prev_end) e->tr_gap += (double)(w[1] - e->tr_prev_end) * 0.01;
        }
        e->tr_prev_end = w[2];
        e->tr_n++;
    }
#endif
    return MC_OK;
}

bool is_pinned_host(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // pageable memory is "invalid value" to the runtime: not an error of ours
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

// Host-buffer batch through the engine's own pinned staging buffer (pageable caller memory, as JACK's buffers are in
// the reference, conv.cu:321-328, 431-437): chunks of Thost blocks, each copied in, processed and copied out in turn.
int process_host_staged(mc_engine* e, const float* in1, const float* in2, float* outL, float* outR, int T) {
    const size_t cap = (size_t)e->Thost * MC_B;
    for (int o = 0; o < T; o += e->Thost) {
        const int n = std::min(e->Thost, T - o);
        const size_t bytes = (size_t)n * MC_B * sizeof(float), off = (size_t)o * MC_B;
        std::memcpy(e->h_io + 0 * cap, in1 + off, bytes);
        std::memcpy(e->h_io + 1 * cap, in2 + off, bytes);
        HIP_TRY(hipMemcpyAsync(e->d_io[0], e->h_io + 0 * cap, bytes, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->d_io[1], e->h_io + 1 * cap, bytes, hipMemcpyHostToDevice, e->stream));
        int rc = run_front(e, e->d_io[0], e->d_io[1], n, nullptr, 0, n, e->d_io[2], e->d_io[3]);
        if (rc) return rc;
        rc = run_back(e, e->d_io[0], e->d_io[1], nullptr, e->d_io[2], e->d_io[3], n);
        if (!rc) rc = fence_post(e);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(e->h_io + 2 * cap, e->d_io[2], bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(e->h_io + 3 * cap, e->d_io[3], bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        std::memcpy(outL + off, e->h_io + 2 * cap, bytes);
        std::memcpy(outR + off, e->h_io + 3 * cap, bytes);
    }
    return MC_OK;
}

// Host-buffer batch with pinned caller memory: the DMA engines read the caller's input buffers directly, and the kernels
// that finish the output store it straight into the caller's output buffers.  Chunks of Tdev blocks; chunk k's copy-in
// (H2D stream) runs under chunk k - 1's kernels (engine stream), over three staging sets.  Returns when the last output
// byte is in outL / outR.
int process_host_pinned(mc_engine* e, const float* in1, const float* in2, float* outL, float* outR, int T) {
    if (!e->pinned) {
        // whole chunks of the second-level transform where it applies, and LONG ones: the copies set the pace, and the
        // link carries 45-48 GB/s each way at once in copies of >= 33 MB but only 26 GB/s in 6.6 MB ones
        // (scripts/pcie_probe.py; 53-57 GB/s one way at a time)
        int tdev = (int)std::min<uint64_t>(mc_preferred_batch(e, std::min(e->Tmax, 32768)), (uint64_t)e->Tmax);
        tdev = std::max(tdev / e->pm * e->pm, e->pm);
        HIP_TRY(make_group(e->pinned, (size_t)tdev * MC_B));
        e->Tdev = tdev;
    }
    PinnedStaging& ps = *e->pinned;
    int k = 0;
    for (int o = 0; o < T; o += e->Tdev, k++) {
        const int n = std::min(e->Tdev, T - o), b = k % 3;
        const size_t bytes = (size_t)n * MC_B * sizeof(float), off = (size_t)o * MC_B;
        const DevArray<float>* d = ps.d_in[b];
        // the staging set is free once chunk k - 3 has been computed (inputs) and copied out (outputs)
        if (k >= 3) HIP_TRY(hipStreamWaitEvent(ps.h2d, ps.ev_comp[b], 0));
        HIP_TRY(hipMemcpyAsync(d[0], in1 + off, bytes, hipMemcpyHostToDevice, ps.h2d));
        HIP_TRY(hipMemcpyAsync(d[1], in2 + off, bytes, hipMemcpyHostToDevice, ps.h2d));
        HIP_TRY(hipEventRecord(ps.ev_h2d[b], ps.h2d));
        HIP_TRY(hipStreamWaitEvent(e->stream, ps.ev_h2d[b], 0));
        // the kernels that finish the output store it straight into the caller's pinned buffers (posted writes over the
        // link): no copy-out, no second copy direction to take turns with the copy-in
        float *hl = nullptr, *hr = nullptr;
        HIP_TRY(hipHostGetDevicePointer((void**)&hl, outL + off, 0));
        HIP_TRY(hipHostGetDevicePointer((void**)&hr, outR + off, 0));
        // (the output goes over the link as posted writes: the partitioned passes store it in whole 1 KB rows, the overlap-save
        // form's output pass in 64-byte pieces - 119 000 against 109 000 x real time: the link prefers the former)
        e->os_hold = true;
        int rc = run_front(e, d[0], d[1], n, nullptr, 0, n, hl, hr);
        e->os_hold = false;
        if (rc) return rc;
        rc = run_back(e, d[0], d[1], nullptr, hl, hr, n);
        if (!rc) rc = fence_post(e);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(ps.ev_comp[b], e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return MC_OK;
}

int process_host(mc_engine* e, const float* in1, const float* in2, float* outL, float* outR, int T) {
    if (!in1 || !in2 || !outL || !outR) return fail(MC_ERR_ARG, "null buffer");
    if (T <= 0) return fail(MC_ERR_ARG, "nblocks %d < 1", T);
    if (T % e->pm) return fail(MC_ERR_ARG, "nblocks %d is not a multiple of the period (%d blocks)", T, e->pm);
    if (is_pinned_host(in1) && is_pinned_host(in2) && is_pinned_host(outL) && is_pinned_host(outR))
        return process_host_pinned(e, in1, in2, outL, outR, T);
    return process_host_staged(e, in1, in2, outL, outR, T);
}

// One JACK period of 512 / 1024 frames (pm = 2 / 4 blocks): the batch pipeline with zero-copy I/O - k_fwd reads the
// period from mapped host memory, k_post writes the output there and raises the completion flag.
int process_period(mc_engine* e, const float* in1, const float* in2, float* outL, float* outR) {
    if (!in1 || !in2 || !outL || !outR) return fail(MC_ERR_ARG, "null buffer");
    if (e->pipe_count) return fail(MC_ERR_STATE, "a sharded batch is still pending");
    {
        int rc = drain_post(e);
        if (rc) return rc;
    }
    const int T = e->pm;
    const size_t cap = (size_t)e->Thost * MC_B;
    period_to_mapped(e, in1, in2, T);
    const bool was_piped = e->pipelined;
    e->pipelined = false;  // a period is finished inside this call
    int rc = run_front(e, e->h_io.dev() + 0 * cap, e->h_io.dev() + 1 * cap, T, nullptr, 0, T);
    if (!rc) rc = run_back(e, e->h_io.dev() + 0 * cap, e->h_io.dev() + 1 * cap, nullptr, e->h_io.dev() + 2 * cap, e->h_io.dev() + 3 * cap, T, true);
    e->pipelined = was_piped;
    if (rc) return rc;
    if (!e->spin_wait) HIP_TRY(hipEventRecord(e->ev_tail, e->stream));
    rc = wait_period(e, e->flag_seq);
    if (rc) return rc;
    copy_period_out(e, outL, outR, T);
    return MC_OK;
}

// One JACK period of 512 / 1024 frames on an unsharded engine: the streaming MAC over partitions >= pm (summed
// speculatively in the shadow of the previous period, as in process_one) and the fused k_tailp.  In the steady state the
// NEXT period's k_tailp is launched behind its sweep one call ahead and parks on the doorbell (as process_one's tail does):
// the call that brings the period writes it through the BAR, rings, and waits - no launch on its critical path.
int process_period_fused(mc_engine* e, const float* in1, const float* in2, float* outL, float* outR) {
    if (!in1 || !in2 || !outL || !outR) return fail(MC_ERR_ARG, "null buffer");
    if (e->pipe_count) return fail(MC_ERR_STATE, "a sharded batch is still pending");
    if (e->sliced) return fail(MC_ERR_STATE, "single-period call on a block-sliced engine (mc_reset first)");
    const int pm = e->pm;
    mc_cc_value cc[2];
    {
        int rc = sample_params(e, cc);
        if (rc) return rc;
    }

    // ---- what a staged period sweeps and what its tail multiplies itself
    struct PPlan {
        ActiveVoice sweep[MC_MAXV];
        int hi[MC_MAXV], nsweep = 0, nsum = 1;
        VoiceSet vset;
    };
    auto make_pplan = [&](const Staged& st, PPlan& pl) {
        std::memset(&pl.vset, 0, sizeof(pl.vset));
        pl.nsweep = 0;
        for (int a = 0; a < st.nact; a++) {
            const int pe = st.act[a].p_end;
            if (pe <= 0) continue;
            pl.vset.vid[pl.vset.n] = st.act[a].v;
            pl.vset.H0[pl.vset.n] = st.act[a].ir0->d_H;
            pl.vset.H1[pl.vset.n] = st.act[a].ir1->d_H;
            pl.vset.n++;
            if (pe > pm) {
                pl.sweep[pl.nsweep] = st.act[a];
                pl.hi[pl.nsweep] = pe;
                pl.nsweep++;
            }
        }
        pl.nsum = std::max(1, pl.nsweep) * kNchunk;
    };
    // partitions >= pm of the pm blocks starting at `blk` pair only with blocks before blk
    auto launch_mac = [&](const PPlan& pl, uint64_t blk) -> int {
        return stamped_sweep(e, pm, [&](unsigned long long* stamps) {
            const int bslot0 = (int)(blk & (uint64_t)(e->ring - 1));
            int swept = 0;
            for (int a = 0; a < pl.nsweep; a++) {
                ActiveVoice av = pl.sweep[a];
                av.uniform = e->gain_change_block[av.v] + (uint64_t)pl.hi[a] <= blk && e->gain_change_block[av.v] < blk;
                launch_mac_stream(e, e->stream, av, pm, pl.hi[a], pm, bslot0, pl.nsum, a * kNchunk, nullptr, stamps);
                swept = std::max(swept, pl.hi[a]);
            }
            return swept;
        });
    };
    auto sweep_or_zero = [&](const PPlan& pl, uint64_t blk) -> int {
        if (pl.nsweep) return launch_mac(pl, blk);
        HIP_TRY(hipMemsetAsync(e->d_part, 0, sizeof(float4) * (size_t)pm * MC_NB * pl.nsum, e->stream));
        return MC_OK;
    };
    int prep_rc = MC_OK;  // first failure of prepare_drop_fft inside launch_tail (checked behind every call)
    auto launch_tail = [&](const Staged& st, const PPlan& pl, uint64_t blk, unsigned seq, bool parked) {
        const unsigned long long* bell = parked ? (e->bar_io ? reinterpret_cast<unsigned long long*>(e->d_bar.get()) : e->hd_bell) : nullptr;
        {
            const int r = prepare_drop_fft(e, st.ctx.vir, st.ctx.predelay);
            if (r != MC_OK && prep_rc == MC_OK) prep_rc = r;
        }
        const TailDrop tdp = make_taildrop(e, st.ctx.vir, st.ctx.predelay);
        // Q8 regime: a parked tail sums its own cut terms while it waits for the period; one launched on arrival gets them from a launch ahead of it
        const bool self_drop = parked && tdp.on && tdp.fft;
        const float* drop = self_drop ? e->d_drop[(blk / (uint64_t)e->pm) & 1] : launch_drop_period(e, tdp, blk, st.ctx.predelay);
        if (self_drop) e->n_drop_carried++;
        auto* launch = pm == 2 ? (self_drop ? launch_tailp<2, true> : launch_tailp<2, false>)
                               : (self_drop ? launch_tailp<4, true> : launch_tailp<4, false>);
        launch(e, st, pl.vset, pl.nsum, blk, seq, tdp, bell, drop);
    };

    // ---- this period: a parked tail staged with the same parameters, or the ordinary launches
    Staged st;
    PPlan pl;
    unsigned my_seq = 0;
    bool relaunch_ok = false;
    if (parked_hit(e, cc, pm)) {
        my_seq = e->pre.seq;
        copy_period_in(e, in1, in2, pm);
        ring_bell(e, my_seq, 0);
        e->pre.valid = false;
        e->n_park_hit++;
        st = e->pre.st;
        make_pplan(st, pl);
        relaunch_ok = true;
        e->spec_valid = false;  // (its sweep has been consumed)
    } else {
        int rc = drain_post(e);
        if (!rc) unpark(e);
        copy_period_in(e, in1, in2, pm);
        if (!rc) rc = retire_epoch(e, cc[0].predelay);
        if (!rc) rc = stage_params(e, pm, cc, &st);
        if (rc) return rc;
        if (st.ctx.pstride != 0) return fail(MC_ERR_STATE, "the blocks of one period must share their parameters");
        make_pplan(st, pl);
        if (!sweep_matches(e, pl.sweep, pl.nsweep, st.ctx.vir, e->t_front)) {
            rc = sweep_or_zero(pl, e->t_front);
            if (rc) return rc;
        }
        e->spec_valid = false;
        my_seq = ++e->flag_seq;
        launch_tail(st, pl, e->t_front, my_seq, false);
        if (prep_rc) return prep_rc;
        HIP_TRY(hipGetLastError());
    }
    if (!e->spin_wait) HIP_TRY(hipEventRecord(e->ev_tail, e->stream));
    e->batch_seq++;
    e->t_front += (uint64_t)pm;
    e->t_abs = e->t_front;

    // ---- the next period: its sweep in the shadow of this one (a speculation the next call checks), and - when nothing
    // is moving - its tail behind the sweep, parked
    if (pl.nsweep) {
        int rc = launch_mac(pl, e->t_front);
        if (rc) return rc;
        remember_sweep(e, pl.sweep, pl.nsweep, st.ctx.vir, e->t_front);
    }
    if (may_park(e, cc)) {
        Staged st_next;
        int rc = stage_params(e, pm, cc, &st_next);  // (steady: advancing the cross-fade by a call changes nothing)
        if (rc) return rc;
        PPlan pl_next;
        make_pplan(st_next, pl_next);
        if (st_next.ctx.pstride == 0 && std::memcmp(&st_next.first, &st.first, sizeof(BlockParams)) == 0 &&
            (pl_next.nsweep == 0 || sweep_matches(e, pl_next.sweep, pl_next.nsweep, st_next.ctx.vir, e->t_front))) {
            if (!pl_next.nsweep) {
                rc = sweep_or_zero(pl_next, e->t_front);
                if (rc) return rc;
            }
            const unsigned seq = ++e->flag_seq;
            launch_tail(st_next, pl_next, e->t_front, seq, true);
            if (prep_rc) return prep_rc;
            HIP_TRY(hipGetLastError());
            note_parked(e, cc, pm, seq, st_next);
        }
    }
    // When the parked tail gave up on its own, the same period is launched the ordinary way.  What was queued behind it worked
    // on a delay line without this period: the next period's parked tail is told to give up, its sweep is forgotten, and this
    // period's own partial sums are summed again (the sweep behind overwrote them)
    auto relaunch = [&](unsigned* seq) -> int {
        copy_period_in(e, in1, in2, pm);  // (a tail launched now reads the plain copy of the period)
        unpark(e);
        e->spec_valid = false;
        int rc = sweep_or_zero(pl, e->t_front - (uint64_t)pm);
        if (rc) return rc;
        *seq = ++e->flag_seq;
        launch_tail(st, pl, e->t_front - (uint64_t)pm, *seq, false);
        if (prep_rc) return prep_rc;
        HIP_TRY(hipGetLastError());
        return MC_OK;
    };
    {
        int rc = await_period(e, wait_period, my_seq, relaunch_ok, relaunch);
        if (rc) return rc;
    }
    copy_period_out(e, outL, outR, pm);
    return MC_OK;
}

}  // namespace

#include "singlefft_host.hip.h"

namespace {

// The mapped I/O buffer of the period calls (4 * Thost blocks), the mapped line of their flags, and the BAR page where the CPU can
// write device memory (see mc_engine::d_bar)
int create_period_io(mc_engine* e) {
    HIP_TRY(e->h_io.alloc(4 * (size_t)e->Thost * MC_B, hipHostMallocMapped));
    HIP_TRY(e->h_flag.alloc(64, hipHostMallocMapped));  // completion word, doorbell, "gave up" word: a line each
    std::memset(e->h_flag, 0, 256);
    if (std::getenv("MCCONV_NO_SPIN")) e->spin_wait = false;
    int large_bar = 0;
    const char* bi = std::getenv("MCCONV_BAR_IO");
    if ((!bi || std::atoi(bi) != 0) && hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, e->device) == hipSuccess && large_bar &&
        e->d_bar.alloc_finegrained(8192) == hipSuccess) {
        HIP_TRY(hipMemset(e->d_bar, 0, 32768));
        e->bar_io = true;
    } else {
        (void)hipGetLastError();
    }
    return MC_OK;
}

int create_engine(mc_engine* e) {
    const mc_config* cfg = &e->cfg;
    e->ph.update([](mc_cc_value (&cc)[2]) {
        mc_default_params(&cc[0]);
        mc_default_params(&cc[1]);
    });
    std::memset(&e->ks, 0, sizeof(e->ks));
    e->Tmax = (int)cfg->max_batch;
    e->Tcap = std::max(e->Tmax, 256);
    e->Pcap = cfg->max_partitions ? (int)cfg->max_partitions : (int)((cfg->n_ref - 1024 + MC_B - 1) / MC_B);
    e->Pstride = (int)next_pow2((uint64_t)round_up(e->Pcap, 16));
    e->ring = (int)next_pow2((uint64_t)e->Pstride + (uint64_t)e->Tcap + 64);  // + reach-back of a block slice (<= 33)
    e->sr = (int)next_pow2((uint64_t)e->Tcap + 4);  // power of two: ring indices are masks in the kernels; a slice + reach-back <= Tmax
    e->wr = (int)next_pow2((uint64_t)MC_MAX_PREDELAY + (uint64_t)e->Tmax * MC_B + 2 * MC_B);
    e->pipelined = cfg->pipeline != 0 && cfg->precision == 0;
    // (pipelined: the forward stage of batch k + 1 writes histories while the post stage of batch k still reads them)
    e->rc = (int)next_pow2(cfg->n_ref / MC_B + (uint64_t)e->Tmax * (e->pipelined ? 2 : 1) + 64);
    e->stream_threshold = cfg->stream_threshold ? (int)cfg->stream_threshold : 48;  // measured crossover (scripts/sweep_T.sh)
    e->half = cfg->precision == 1;
    if (e->half) e->stream_threshold = e->Tmax + 1;  // the fp16 MAC is the streaming sweep
    // (at least 8 blocks: the fast-FIR form sends the last 2^levels blocks of a batch through the streaming kernel)
    e->Tstream = std::min(e->half ? e->Tmax : e->Tcap, std::max(8, e->stream_threshold - 1));

    if (const char* v = std::getenv("MCCONV_TD_FFT")) e->td_fft = std::atoi(v) != 0;
    HIP_TRY(e->own_stream.create(hipStreamNonBlocking));
    e->stream = e->own_stream;
    if (e->cfg.form == 1) {  // the reference's own shape: none of the partitioned engine's state
        HIP_TRY(e->d_tw.alloc(FFT_N));
        {
            std::vector<float2> tw;
            host_twiddles(tw);
            HIP_TRY(hipMemcpy(e->d_tw, tw.data(), sizeof(float2) * FFT_N, hipMemcpyHostToDevice));
        }
        e->Thost = 4;  // the mapped buffer holds one period
        const int rc = create_period_io(e);
        return rc ? rc : sf_create(e);
    }
    HIP_TRY(e->d_fdl.alloc((size_t)MC_NB * e->ring));
    if (e->half) HIP_TRY(e->d_fdl16.alloc((size_t)MC_NB * e->ring));
    HIP_TRY(e->d_slotgain.alloc((size_t)MC_MAXV * e->ring));
    // >= 8 planes of 256 blocks; the fast-FIR form writes three half-rate sequences (1.5 x the blocks, + a tile each)
    HIP_TRY(e->d_Ybuf[0].alloc((size_t)MC_NB * y_capacity(e)));
    if (!e->half) HIP_TRY(e->d_Ycbuf[0].alloc((size_t)MC_NB * e->Tcap));
    HIP_TRY(e->d_tailbuf[0].alloc((size_t)8 * MC_NB * kNchunk * MC_MAXV));
    e->d_Y = e->d_Ybuf[0];
    e->d_Yc = e->d_Ycbuf[0];
    e->d_tail = e->d_tailbuf[0];
    if (e->pipelined) {
        HIP_TRY(e->post_stream.create(hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) {
            HIP_TRY(e->ev_mac[i][0].create(hipEventDisableTiming));
            HIP_TRY(e->ev_mac[i][1].create(hipEventDisableTiming));
            HIP_TRY(e->ev_corr[i].create(hipEventDisableTiming));
            HIP_TRY(e->ev_post[i].create(hipEventDisableTiming));
        }
        HIP_TRY(e->d_Ybuf[1].alloc((size_t)MC_NB * y_capacity(e)));
        HIP_TRY(e->d_Ycbuf[1].alloc((size_t)MC_NB * e->Tcap));
        HIP_TRY(e->d_tailbuf[1].alloc((size_t)8 * MC_NB * kNchunk * MC_MAXV));
    }
    HIP_TRY(e->d_partbuf[0].alloc((size_t)e->Tstream * MC_NB * kNchunk * MC_MAXV));
    e->d_part = e->d_partbuf[0];
    if (cfg->pipeline != 0 && cfg->precision == 0)
        HIP_TRY(e->d_partbuf[1].alloc((size_t)e->Tstream * MC_NB * kNchunk * MC_MAXV));
    HIP_TRY(e->d_sums.alloc((size_t)e->Tmax * kPipe));
    HIP_TRY(e->d_seg.alloc((size_t)e->sr * 2 * FFT_N));
    HIP_TRY(e->d_wet.alloc(2 * (size_t)e->wr));
    HIP_TRY(e->d_cring.alloc(4 * (size_t)e->rc));
    HIP_TRY(e->d_wring.alloc(4 * (size_t)e->rc));
    HIP_TRY(e->d_ctot.alloc(4 * (size_t)((e->Tmax + 255) / 256 + 1)));
    HIP_TRY(e->d_cflag.alloc((size_t)((e->Tmax + 255) / 256 + 2)));
    HIP_TRY(hipMemset(e->d_cflag, 0, sizeof(unsigned) * e->d_cflag.size()));
    e->d_cticket = e->d_cflag + e->d_cflag.size() - 1;
    e->rr = (int)next_pow2(cfg->n_ref);
    HIP_TRY(e->d_res_mac.alloc(2 * (size_t)e->rr));
    HIP_TRY(e->d_res_fix.alloc(2 * (size_t)e->rr));
    e->xr = (int)next_pow2(cfg->n_ref + (uint64_t)e->Tmax * MC_B * (e->pipelined ? 2 : 1) + MC_MAX_PREDELAY + 1024);
    HIP_TRY(e->d_xhist.alloc(2 * (size_t)e->xr));
    HIP_TRY(e->d_gring.alloc((size_t)MC_MAXV * e->rc));
    HIP_TRY(e->d_ptab.alloc((size_t)e->Tmax * kPipe));
    HIP_TRY(e->d_tw.alloc(FFT_N));
    e->Thost = std::min(e->Tmax, 16384);  // host-buffer calls with pageable buffers stage through pinned memory in chunks of this
    for (int i = 0; i < 4; i++) HIP_TRY(e->d_io[i].alloc((size_t)e->Thost * MC_B));
    HIP_TRY(e->d_tailform.alloc(2));
    HIP_TRY(hipMemset(e->d_tailform, 0, 2 * sizeof(unsigned)));
    if (const char* f = std::getenv("MCCONV_TAIL_FORM")) e->tail_form = !std::strcmp(f, "td") ? 1 : !std::strcmp(f, "fd") ? 2 : 0;
    {
        const int rc = create_period_io(e);
        if (rc) return rc;
    }
    e->h_bell = reinterpret_cast<unsigned long long*>(e->h_flag + 16);
    e->hd_bell = reinterpret_cast<unsigned long long*>(e->h_flag.dev() + 16);
    e->h_exited = e->h_flag + 32;
    e->hd_exited = e->h_flag.dev() + 32;
    if (std::getenv("MCCONV_NO_PARK")) e->park = false;
    if (const char* pm = std::getenv("MCCONV_PARK_MS")) e->park_ticks = (unsigned long long)std::max(1, std::atoi(pm)) * 100000ull;
    HIP_TRY(e->d_done_ctr.alloc(1));
    HIP_TRY(hipMemset(e->d_done_ctr, 0, sizeof(unsigned)));
    if (e->bar_io && e->spin_wait) {
        HIP_TRY(e->h_gran.alloc(2 * MC_B, hipHostMallocMapped));
        std::memset(e->h_gran, 0, sizeof(unsigned long long) * 2 * MC_B);
        e->tio = true;
    }
    for (int i = 0; i < kStageBufs; i++) {
        HIP_TRY(e->h_ptab[i].alloc((size_t)e->Tmax, hipHostMallocDefault));
        HIP_TRY(e->ptab_ev[i].create(hipEventDisableTiming));
    }
    HIP_TRY(e->ev_tail.create(hipEventDisableTiming));
    for (int i = 0; i < 2; i++) HIP_TRY(e->d_part_jack[i].alloc((size_t)MC_NB * kNchunk * MC_MAXV));
    for (int i = 0; i < 2; i++) HIP_TRY(e->d_drop[i].alloc(2 * 4 * MC_B));
    if (const char* f2 = std::getenv("MCCONV_FFT2")) e->fft2 = std::atoi(f2) != 0;
    if (const char* g2 = std::getenv("MCCONV_FFT2_FUSED")) e->fft2_fused = std::atoi(g2) != 0;
    if (const char* tm = std::getenv("MCCONV_FFT2_WORK")) e->fft2_work = std::max<int64_t>(1, std::atoll(tm));
    if (const char* os = std::getenv("MCCONV_OS")) e->os_on = std::atoi(os) != 0;
    if (const char* os = std::getenv("MCCONV_OS_MIN")) e->os_min_blocks = std::max(1, std::atoi(os));
    if (const char* fl = std::getenv("MCCONV_FFA_LEVELS")) e->ffa_levels = std::max(0, std::min(3, std::atoi(fl)));
    {
        std::vector<float2> tw;
        host_twiddles(tw);
        HIP_TRY(hipMemcpy(e->d_tw, tw.data(), sizeof(float2) * FFT_N, hipMemcpyHostToDevice));
    }
    return zero_state(e);
}

}  // namespace

extern "C" {

uint32_t mc_abi_version(void) { return MC_ABI_VERSION; }
const char* mc_last_error(void) { return g_err; }

void mc_default_config(mc_config* cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = sizeof(mc_config);
    cfg->device = -1;
    cfg->n_ref = 512 * 256;  // CONV_DEFAULT_FFTSIZE, conv.h:10-12
    cfg->max_batch = 256;
    cfg->compat = 1;
}

void mc_default_params(mc_cc_value* v) {
    if (!v) return;
    v->select = 0;  // conv.h:40-48
    v->predelay = 0;
    v->speed = 100;
    v->vsteps = 0;
    v->dry = 0.5f;
    v->wet = 0.5f;
    v->panDry = 0.0f;
    v->panWet = 0.0f;
    v->level = 1.0f;
}

int mc_create(const mc_config* cfg, mc_engine** out) {
    if (!cfg || !out) return fail(MC_ERR_ARG, "null argument");
    if (cfg->struct_size != sizeof(mc_config)) return fail(MC_ERR_ARG, "mc_config size mismatch (%u vs %zu)", cfg->struct_size, sizeof(mc_config));
    if (cfg->n_ref < 4096 || (cfg->n_ref & (cfg->n_ref - 1))) return fail(MC_ERR_ARG, "n_ref must be a power of two >= 4096");
    if (cfg->n_ref > (1ull << 26)) return fail(MC_ERR_ARG, "n_ref too large");
    if (cfg->max_batch < 1 || cfg->max_batch > 1048576) return fail(MC_ERR_ARG, "max_batch must be in [1, 1048576]");
    if ((cfg->part_begin % 16) || (cfg->part_end % 16)) return fail(MC_ERR_ARG, "partition shard bounds must be multiples of 16");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(MC_ERR_HIP, "no HIP device");
    int dev = cfg->device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    if (dev >= ndev) return fail(MC_ERR_ARG, "device %d out of range (%d devices)", dev, ndev);
    HIP_TRY(hipSetDevice(dev));
    const uint32_t period = cfg->period ? cfg->period : MC_BLOCK;
    if (period != 256 && period != 512 && period != 1024) return fail(MC_ERR_ARG, "period must be 256, 512 or 1024 frames");
    if (cfg->max_batch % (period / MC_BLOCK)) return fail(MC_ERR_ARG, "max_batch must be a multiple of period / 256");
    uint32_t form = cfg->form;
    {
        const char* fm = std::getenv("MCCONV_FORM");  // lets an unmodified host pick the form: "single" / "partitioned"
        if (fm && !std::strcmp(fm, "single")) form = 1;
        else if (fm && !std::strcmp(fm, "partitioned")) form = 0;
    }
    if (form > 1) return fail(MC_ERR_ARG, "mc_config.form must be 0 (partitioned) or 1 (single transform)");

    // everything the engine holds is an owner (owned.h): whatever create_engine had made when it failed goes with the engine
    mc_engine* e = new (std::nothrow) mc_engine();
    if (!e) return fail(MC_ERR_NOMEM, "out of host memory");
    e->cfg = *cfg;
    e->cfg.form = form;
    e->device = dev;
    e->pm = (int)(period / MC_BLOCK);
    const int rc = create_engine(e);
    if (rc) {
        mc_destroy(e);
        return rc;
    }
    *out = e;
    return MC_OK;
}

void mc_destroy(mc_engine* e) {
    if (!e) return;
#ifdef MC_JACK_TRACE
    if (e->tr_n > 100) {
        const double n = (double)(e->tr_n - 100);
        fprintf(stderr, "mcconv JACK trace over %ld periods (us): entry -> launches issued %.2f, -> flag seen %.2f, -> return %.2f; k_tail1 start -> output issued %.2f (%.0f shader clocks; first barrier %.0f, sums done %.0f, second barrier %.0f), -> end %.2f, "
                        "end of the previous k_tail1 -> start of this one %.2f\n", e->tr_n - 100, e->tr_launch / n, e->tr_flag / n, e->tr_total / n, e->tr_out / n, e->tr_clk / n, e->tr_c[0] / n, e->tr_c[1] / n, e->tr_c[2] / n, e->tr_kernel / n, e->tr_gap / n);
    }
#endif
    (void)hipSetDevice(e->device);
    unpark(e);
    // nothing the engine issued is still running when its owners (owned.h) let go
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    (void)e->own_stream.sync();
    (void)e->post_stream.sync();
    if (e->os_side) (void)e->os_side->stream.sync();
    if (e->pinned) (void)e->pinned->h2d.sync();
    delete e;
}

int mc_reset(mc_engine* e) {
    if (!e) return fail(MC_ERR_ARG, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    return e->sf ? sf_zero(e) : zero_state(e);
}

int mc_set_period(mc_engine* e, uint32_t nframes) {
    if (!e) return fail(MC_ERR_ARG, "null engine");
    if (nframes != 256 && nframes != 512 && nframes != 1024) return fail(MC_ERR_ARG, "period must be 256, 512 or 1024 frames");
    const int pm = (int)(nframes / MC_BLOCK);
    if (e->Tmax % pm) return fail(MC_ERR_ARG, "max_batch %d is not a multiple of %d blocks", e->Tmax, pm);
    if (pm == e->pm) return MC_OK;
    HIP_TRY(hipSetDevice(e->device));
    e->pm = pm;
    return e->sf ? sf_zero(e) : zero_state(e);  // the per-call semantics change: start from the cold state
}

}  // extern "C"

namespace {
// the tail step of a load as load_ir and shape_stage take it: the plan over the frames at the session's rate, and the mode
struct TailStep {
    TailPlan plan;
    bool extend;
};

// the room of a synthesised load as load_ir and shape_stage take it: the plan, the images the device kept per channel, and
// with `banded` the bands of mc_ir_room_bands, which are then what is rendered; with plan.headed the twelve numbers of
// mc_ir_room_head_info
struct RoomStep {
    RoomPlan plan;
    uint32_t kept[2];
    bool banded;
    RoomBands bands;
    double head[12];
};

// the plate of a synthesised load as load_ir and shape_stage take it: the checked plate with its table (irplate.hip.h)
struct PlateStep {
    PlatePlan plan;
};

// the spring tank of a synthesised load as load_ir and shape_stage take it: the checked spring with its constants (irspring.hip.h)
struct SpringStep {
    SpringPlan plan;
};

// One load as load_ir and shape_stage take it: where the frames come from, and the steps they go through on the device.  The
// entry points fill it in by name; a null pointer is a source that is not this load's, or a step that is off.
struct IrLoad {
    // -- the source: `frames` frames from exactly one of lr, syn and swp
    const float* lr = nullptr;         // host frames, interleaved (mc_load_ir and everything built on it)
    uint64_t frames = 0;               // of lr; with syn its F, with swp its F (the frames of the IR, not of the recording)
    const uint32_t* rs = nullptr;      // {IR rate, session rate}: lr's frames are converted on the device (resample.hip.h) before
                                       // anything else sees them; null = they are at the session's rate (the reference)
    const SynPlan* syn = nullptr;      // mc_synth_ir (irsynth.hip.h): the frames are generated on the device
    RoomStep* room = nullptr;          // mc_synth_ir_room (irroom.hip.h; with syn): its reflections are added to the generated
                                       // frames, and the kept counts are filled in; room->banded: once per band of
                                       // room->bands, joined by the band split (mc_synth_ir_room_bands)
    const PlateStep* plate = nullptr;  // mc_synth_ir_plate (irplate.hip.h; with syn and without room): the sum of its modes is added
                                       // to the generated frames
    const SpringStep* spring = nullptr;  // mc_synth_ir_spring (irspring.hip.h; with syn and without room and plate): the tank's
                                         // response is added to the generated frames
    const SweepSource* swp = nullptr;  // mc_load_ir_sweep (irsweep.hip.h): the frames are deconvolved on the device from its recording
    // -- the steps, in the order they run.  Any of tail, eq, damp, syn and swp needs the shape, which may have everything off
    const TailStep* tail = nullptr;      // step 1a, between the source and the shaping (irtail.hip.h; tail->plan.F = the frames at the session's rate)
    const PhaseStep* phase = nullptr;    // step 1b, after the tail step (irphase.hip.h; phase->F = the frames the tail step hands on)
    const FilterStep* filter = nullptr;  // step 1c, after the phase step (irfilter.hip.h; filter->F = the frames the phase step hands on)
    const MatchStep* match = nullptr;    // step 1d, after the filter step (irmatch.hip.h; match->F = the frames the filter step hands on)
    const PartsStep* parts = nullptr;    // step 1e, after the match step (irparts.hip.h; parts->F = the frames the match step hands on)
    const mc_ir_shape* shape = nullptr;  // applied on the device after the conversion (irshape.hip.h)
    const IeqCascade* eq = nullptr;      // the bands of mc_load_ir_eq (ireq.hip.h); with damp it may hold no band
    const DampPlan* damp = nullptr;      // the damping of mc_load_ir_damped (irdamp.hip.h; needs eq)
};

// what the shaping stage hands back: n taps on the device that the caller owns, mc_ir_info's sums of them and mc_ir_shape_info's numbers
struct ShapedTaps {
    float2* d_taps = nullptr;
    uint64_t n = 0;
    double sums[4] = {0, 0, 0, 0}, info[8];
    double phase[8];    // mc_ir_phase_info's numbers, with IrLoad::phase
    double filter[10];  // mc_ir_filter_info's numbers, with IrLoad::filter
    MatchFacts match;   // mc_ir_match_info's numbers and mc_ir_match_curve's arrays, with IrLoad::match
    double parts[10];   // mc_ir_parts_info's numbers, with IrLoad::parts
};

// The stream idle and out of the JACK path, before the kernels of a load or of a measurement go onto it.  (The single-transform
// form has no post stream and parks no period.)
int quiesce(mc_engine* e) {
    HIP_TRY(hipSetDevice(e->device));
    int rc = e->sf ? MC_OK : drain_post(e);
    if (!rc && !e->sf) unpark(e);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return MC_OK;
}

// The shaped load's own stage (irshape.hip.h): all `conv` frames of ld's source at the session's rate on the device, shaped
// into a new buffer of out->n <= cap taps.  Nothing of the engine's IRs is touched here.  A sweep's recording is uploaded to a
// temporary buffer freed after the stage, as its weight table is; the tail step turns the conv frames into tail->plan.Fp frames
// in a buffer of their own, the phase step those into as many frames in another, the filter step those into filter->Fo, the match step those into match->Fo, and the parts step those into parts->Fo.
int shape_stage(mc_engine* e, const IrLoad& ld, uint64_t conv, uint64_t cap, ShapedTaps* out) {
    DevArray<float2> d_x, d_rec;
    DevArray<double> d_u;
    HIP_TRY(d_x.alloc(conv));
    double unused[4];
    hipError_t er = ld.swp  ? swp_generate(e->stream, *ld.swp, d_x, d_rec, d_u)
                    : ld.syn && ld.room && ld.room->banded ? room_generate_bands(e->stream, *ld.syn, ld.room->bands, d_x, ld.room->kept)
                    : ld.syn && ld.room ? room_generate(e->stream, *ld.syn, ld.room->plan, d_x, ld.room->kept)
                    : ld.syn && ld.plate ? plate_generate(e->stream, *ld.syn, ld.plate->plan, d_x)
                    : ld.syn && ld.spring ? spring_generate(e->stream, *ld.syn, ld.spring->plan, d_x)
                    : ld.syn ? syn_generate(e->stream, *ld.syn, d_x)
                    : ld.rs ? rs_convert(e->stream, ld.rs[0], ld.rs[1], ld.lr, ld.frames, d_x, conv, unused)
                            : hipMemcpy(d_x, ld.lr, sizeof(float2) * conv, hipMemcpyHostToDevice);
    // one step: its Fo frames into a buffer of their own, which then takes d_x's place (run waits for the stream: d_x is free after it)
    const auto step = [&](uint64_t Fo, auto&& run) {
        if (er != hipSuccess) return;
        DevArray<float2> d_y;
        er = d_y.alloc(Fo);
        if (er == hipSuccess) er = run(d_y);
        if (er == hipSuccess) {
            d_x = std::move(d_y);
            conv = Fo;
        } else {
            (void)hipStreamSynchronize(e->stream);
        }
    };
    if (ld.tail) step(ld.tail->plan.Fp, [&](float2* d_y) { return tail_run(e->stream, d_x, d_y, ld.tail->plan, ld.tail->extend); });
    if (ld.phase) step(conv, [&](float2* d_y) { return phase_run(e->stream, d_x, d_y, *ld.phase, out->phase); });
    if (ld.filter) step(ld.filter->Fo, [&](float2* d_y) { return filter_run(e->stream, d_x, d_y, *ld.filter, out->filter); });
    if (ld.match) step(ld.match->Fo, [&](float2* d_y) { return match_run(e->stream, d_x, d_y, *ld.match, &out->match); });
    if (ld.parts) step(ld.parts->Fo, [&](float2* d_y) { return parts_run(e->stream, d_x, d_y, *ld.parts, out->parts); });
    if (er == hipSuccess) er = ish_shape(e->stream, d_x, conv, cap, *ld.shape, &out->d_taps, &out->n, out->sums, out->info, ld.eq, ld.damp);
    if (ld.swp && er != hipSuccess) (void)hipStreamSynchronize(e->stream);  // (the correlation may still be reading them)
    if (er != hipSuccess) return fail(MC_ERR_HIP, "IR shaping failed: %s", hipGetErrorString(er));
    if (!out->n) return fail(MC_ERR_ARG, "the shape leaves no frame of the IR (start %llu, %llu frames at the session's rate)",
                             (unsigned long long)ld.shape->start, (unsigned long long)conv);
    return MC_OK;
}

// What the mc_ir_*_info getters report of the load `ld` that stored `taps` taps; st = what the shaping stage handed back, whose
// numbers of a step are read when ld has that step.  Every kind is written, so nothing of an earlier load onto the same index
// stays behind.
void note_load(IrEntry& ir, const IrLoad& ld, uint64_t taps, const ShapedTaps& st) {
    const double *sinfo = st.info, *pinfo = st.phase, *finfo = st.filter;
    for (IrFact& f : ir.facts) f.on = false;
    const auto put = [&ir](IrFactKind kind, std::initializer_list<double> v) {
        ir.facts[kind].on = true;
        std::copy(v.begin(), v.end(), ir.facts[kind].v);
    };
    if (ld.shape) put(FACT_SHAPE, {sinfo[0], sinfo[1], sinfo[2], sinfo[3], sinfo[4], sinfo[5], sinfo[6], sinfo[7]});
    if (const DampPlan* d = ld.damp) {
        int decays = 0;
        for (int j = 0; j <= d->X; j++) decays += d->t60[j] != 0;
        put(FACT_DAMP, {(double)d->X, (double)std::min<uint64_t>(d->origin, taps), (double)decays, 0.0});
    }
    if (const SynPlan* s = ld.syn) put(FACT_SYNTH, {(double)s->F, (double)s->n_early, (double)std::min<uint64_t>(s->late_start, s->F), 0.0});
    if (const SweepSource* s = ld.swp) put(FACT_SWEEP, {(double)s->plan.N, (double)s->M, (double)s->F, (double)s->offset});
    if (ld.tail) {
        const TailPlan& t = ld.tail->plan;
        put(FACT_TAIL, {(double)t.touched, (double)t.F, (double)t.Fp, (double)t.first});
    }
    if (ld.phase) put(FACT_PHASE, {pinfo[0], pinfo[1], pinfo[2], pinfo[3], pinfo[4], pinfo[5], pinfo[6], pinfo[7]});
    if (ld.filter) put(FACT_FILTER, {finfo[0], finfo[1], finfo[2], finfo[3], finfo[4], finfo[5], finfo[6], finfo[7], finfo[8], finfo[9]});
    ir.match_curve.clear();
    if (ld.match) {
        const double* m = st.match.info;
        put(FACT_MATCH, {m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11]});
        ir.match_curve = st.match.curve;
    }
    if (ld.parts) {
        const double* p = st.parts;
        put(FACT_PARTS, {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]});
    }
    if (ld.room) {
        const RoomPlan& r = ld.room->plan;
        put(FACT_ROOM, {(double)r.N, (double)ld.room->kept[0], (double)ld.room->kept[1], r.tau[0], r.tau[1], (double)r.E, (double)r.complete, 0.0});
        if (r.mics) {
            double m[8];
            room_mics_report(r, m);
            put(FACT_ROOM_MICS, {m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7]});
        }
        if (r.headed) {
            const double* h = ld.room->head;
            put(FACT_ROOM_HEAD, {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], h[10], h[11]});
        }
        if (ld.room->banded) {
            const double* b = ld.room->bands.report;
            put(FACT_ROOM_BANDS, {b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8], b[9], b[10], b[11], b[12], b[13], b[14], b[15]});
        }
    }
    if (ld.plate) {
        const PlatePlan& p = ld.plate->plan;
        put(FACT_PLATE, {(double)p.M, (double)p.nonzero[0], (double)p.nonzero[1], (double)p.E, p.lo, p.hi, p.kappa, 0.0});
    }
    if (ld.spring) {
        ir.facts[FACT_SPRING].on = true;
        spring_numbers(ld.spring->plan, ir.facts[FACT_SPRING].v);
    }
}

// Every load: the entry points check their arguments, describe the load (IrLoad) and come here.  nframes = the period the
// engine's n_ref was sized for.  A load without a shape is the reference's (Convolution::prepare): lr, converted first with rs.
int load_ir(mc_engine* e, uint64_t idx, uint64_t nframes, const IrLoad& ld) {
    // Convolution::prepare, conv.cu:207-253
    const float* const lr = ld.lr;
    const uint64_t frames = ld.frames;
    const uint32_t* const rs = ld.rs;
    const bool sh = ld.shape != nullptr;
    if (!e || (!lr && !ld.syn && !ld.swp)) return fail(MC_ERR_ARG, "null argument");
    if (idx >= (uint64_t)kMaxIrs) return fail(MC_ERR_ARG, "IR index %llu >= %d", (unsigned long long)idx, kMaxIrs);
    if (nframes >= e->cfg.n_ref) return fail(MC_ERR_ARG, "nframes >= n_ref");
    if (frames == 0) return fail(MC_ERR_ARG, "empty IR");
    const uint64_t conv = rs ? rs_out_frames(rs_geom(rs[0], rs[1]), frames) : frames;  // frames at the session's rate
    HIP_TRY(hipSetDevice(e->device));
    DevArray<float2> d_lr;  // the taps {L, R}
    ShapedTaps st;  // (without a shape, st.sums takes the sums of a conversion)
    if (sh) {
        int rc = quiesce(e);
        if (!rc) rc = shape_stage(e, ld, conv, e->cfg.n_ref - nframes, &st);
        if (rc) return rc;
        d_lr.adopt(st.d_taps, st.n);
    }
    if (e->sf) {
        const int rc = sf_load_ir(e, idx, lr, frames, nframes, rs, st.d_taps, st.n, st.sums);
        if (rc) return rc;
        note_load(e->irs[idx], ld, st.n, st);
        return MC_OK;
    }
    const uint64_t n = sh ? st.n : std::min<uint64_t>(conv, e->cfg.n_ref - nframes);  // conv.cu:239
    const int P = (int)((n + MC_B - 1) / MC_B);
    if (P > e->Pcap) return fail(MC_ERR_ARG, "IR needs %d partitions, engine capacity is %d", P, e->Pcap);
    IrEntry& ir = e->irs[idx];
    if (!sh)  // (a shaped load did this before its stage)
        if (const int rc = quiesce(e)) return rc;
    hipError_t er = hipStreamSynchronize(e->stream);
    if (er == hipSuccess && !ir.d_H) er = ir.d_H.alloc((size_t)MC_NB * e->Pstride);
    if (er == hipSuccess && !sh) er = d_lr.alloc(n);
    if (er != hipSuccess) return fail(MC_ERR_HIP, "IR preparation failed: %s", hipGetErrorString(er));
    if (!sh)
        er = rs ? rs_convert(e->stream, rs[0], rs[1], lr, frames, d_lr, n, st.sums)
                : hipMemcpy(d_lr, lr, sizeof(float) * 2 * n, hipMemcpyHostToDevice);
    if (er == hipSuccess) er = ir.d_H.zero(e->stream);
    if (er == hipSuccess) {
        const float* const taps = reinterpret_cast<const float*>(d_lr.get());
        hipLaunchKernelGGL(k_fwd<false>, dim3((P + FWD_TILE - 1) / FWD_TILE), dim3(XF_THREADS), 0, e->stream, taps, taps + 1, 2, (int64_t)n, P,
                           ir.d_H, e->Pstride, 0, (const BlockParams*)nullptr, 0, (float4*)nullptr, (float4*)nullptr, e->d_tw,
                           (uint2*)nullptr, (float*)nullptr, 0, (float4*)nullptr, 0, (int64_t)0, 0, P, P, 0, 0, DropAhead(), 0);
        er = hipGetLastError();
    }
    if (er == hipSuccess) er = hipStreamSynchronize(e->stream);
    if (er != hipSuccess) return fail(MC_ERR_HIP, "IR preparation failed: %s", hipGetErrorString(er));
    ir.d_Htail.reset();
    ir.d_h = std::move(d_lr);  // the truncated taps stay on the device for the Q8 pass
    invalidate_derived(ir);
    e->ir_gen++;
    for (int l = 0; l < 3; l++) ir.d_Hp[l].reset();  // (a reloaded IR gives its fast-FIR components back; the stream is idle here)
    if (e->half) {
        // scaled fp16 copy: one power-of-two scale per IR puts the largest bin near 2^13 (half max 65504);
        // a 60 dB decay then still sits ~2^3 above the smallest normal half
        const size_t nel = (size_t)MC_NB * e->Pstride;
        std::vector<float> host(nel * 4);
        HIP_TRY(hipMemcpy(host.data(), ir.d_H, sizeof(float4) * nel, hipMemcpyDeviceToHost));
        float mx = 0.f;
        for (float v : host) mx = std::max(mx, std::fabs(v));
        int ex = 0;
        if (mx > 0.f) std::frexp(mx, &ex);
        ir.scale16 = std::ldexp(1.0f, std::min(13 - ex, kScale16MaxExp));
        if (!ir.d_H16) HIP_TRY(ir.d_H16.alloc(nel));
        hipLaunchKernelGGL(k_to_half, dim3(1024), dim3(256), 0, e->stream, ir.d_H, ir.d_H16, nel, ir.scale16);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    double s[4] = {0, 0, 0, 0};
    if (rs || sh)
        std::memcpy(s, st.sums, sizeof(s));  // (summed on the device: the converted and the shaped taps never come to the host)
    else
        for (uint64_t m = 0; m < n; m++) {
            const double sg = (m & 1) ? -1.0 : 1.0;
            s[0] += lr[2 * m];
            s[1] += lr[2 * m + 1];
            s[2] += sg * lr[2 * m];
            s[3] += sg * lr[2 * m + 1];
        }
    std::memcpy(ir.sums, s, sizeof(s));
    ir.taps = n;
    ir.P = P;
    note_load(ir, ld, n, st);
    if ((int)idx + 1 > e->nirs) e->nirs = (int)idx + 1;
    e->spec_valid = e->dspec.valid = false;
    e->uniform_valid[0] = e->uniform_valid[1] = false;
    return MC_OK;
}

// The damp, eq and shape arguments of a load as every entry point from mc_load_ir_damped on takes them: damping is on with a
// crossover, a null eq is the default (no band) and a null shape the default (everything off).  The cascade and the plan are
// for the session's rate; damping needs the cascade even with no band on (ieq_finish then runs with none).
struct IrSteps {
    mc_ir_shape shape;
    IeqCascade cs;
    DampPlan pl;
    bool on, damping;  // an eq band is on; the damping is on
    void into(IrLoad& ld) const {
        ld.shape = &shape;
        ld.eq = on || damping ? &cs : nullptr;
        ld.damp = damping ? &pl : nullptr;
    }
};

// Checks damp if it is on, then eq, then shape, and fills *st; the message of the first check that fails, null when all pass.
// No engine and no HIP call.  (mc_load_ir_eq and mc_load_ir_shaped do not come here: they check the eq or the shape before the
// rates and the frames, and with nothing on they are a plainer load whose own checks then speak.)
const char* resolve_steps(const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, uint32_t ir_rate, uint32_t session_rate,
                          IrSteps* st) {
    st->damping = damp && damp->n_xovers;
    if (st->damping)
        if (const char* bad = damp_check(damp, ir_rate, session_rate)) return bad;
    mc_ir_eq noeq;
    mc_default_ir_eq(&noeq);
    if (!eq) eq = &noeq;
    int on = 0;
    if (const char* bad = ieq_check(eq, ir_rate, session_rate, &on)) return bad;
    st->on = on != 0;
    mc_default_ir_shape(&st->shape);
    if (shape) {
        if (const char* bad = ish_check(shape)) return bad;
        st->shape = *shape;
    }
    st->cs.bands = 0;
    st->pl = DampPlan{};
    if (st->on || st->damping) st->cs = ieq_cascade(*eq, session_rate);
    if (st->damping) st->pl = damp_plan(*damp, session_rate);
    return nullptr;
}

// The mc_ir_*_info getters (shape, damp, synth, sweep, tail, phase, filter, match, parts, room, room mics, room bands, room head, plate, spring): out = the first `count` numbers of what
// note_load kept of that kind, or MC_ERR_STATE with "IR <idx> <was_not>" when the last load had none
int ir_fact(const mc_engine* e, uint64_t idx, IrFactKind kind, int count, const char* was_not, double* out) {
    if (!e || !out || idx >= (uint64_t)kMaxIrs || !(e->irs[idx].d_H || e->irs[idx].d_S)) return fail(MC_ERR_ARG, "IR %llu not loaded", (unsigned long long)idx);
    const IrFact& f = e->irs[idx].facts[kind];
    if (!f.on) return fail(MC_ERR_STATE, "IR %llu %s", (unsigned long long)idx, was_not);
    std::copy(f.v, f.v + count, out);
    return MC_OK;
}

// What a measurement (mc_ir_decay, mc_ir_floor, mc_ir_density, mc_ir_iacc, mc_ir_sti, mc_ir_response) does once the entry point has checked its query
// and its pointers: the stored taps of IR idx, then work(n), the query's bounds on the work that n taps make (a message, or null),
// both without a HIP call; then the stream idle, run(d_x, n), and a failure of it under the measurement's `name`.
template <class Work, class Run>
int measure(mc_engine* e, uint64_t idx, const char* name, Work&& work, Run&& run) {
    if (e->sf) return fail(MC_ERR_STATE, "the single-transform form keeps no taps");
    if (idx >= (uint64_t)kMaxIrs || !e->irs[idx].d_h || !e->irs[idx].taps) return fail(MC_ERR_ARG, "IR not loaded");
    const uint64_t n = e->irs[idx].taps;
    if (const char* bad = work(n)) return fail(MC_ERR_ARG, "%s", bad);
    if (const int rc = quiesce(e)) return rc;
    const hipError_t er = run(e->irs[idx].d_h, n);
    if (er != hipSuccess) return fail(MC_ERR_HIP, "%s measurement failed: %s", name, hipGetErrorString(er));
    return MC_OK;
}
// (a measurement whose work has no bound)
template <class Run>
int measure(mc_engine* e, uint64_t idx, const char* name, Run&& run) {
    return measure(e, idx, name, [](uint64_t) { return (const char*)nullptr; }, run);
}

// the tail step of a checked mc_ir_tail that is on, over F frames at the session's rate
TailStep tail_step(const mc_ir_tail& tail, uint32_t rate, uint64_t F) { return TailStep{tail_plan(tail, rate, F), tail.mode == MC_TAIL_EXTEND}; }

// The arguments of steps 1a to 1e as an entry point receives them.  An entry point fills in by name what it takes; normalise()
// is the one place that looks at the switches: a step that is off becomes a null pointer, whatever else its struct holds.
struct StepRequest {
    const mc_ir_tail* tail = nullptr;
    const mc_ir_phase* phase = nullptr;
    const mc_ir_filter* filter = nullptr;
    const float* filter_lr = nullptr;
    uint64_t filter_frames = 0;
    const mc_ir_match* match = nullptr;
    const float* target_lr = nullptr;
    uint64_t target_frames = 0;
    const mc_ir_parts* parts = nullptr;
    StepRequest& normalise() {
        if (tail && tail->mode == MC_TAIL_OFF) tail = nullptr;
        if (phase && phase->mode == MC_PHASE_OFF) phase = nullptr;
        if (filter && filter->op == MC_FILTER_OFF) filter = nullptr;
        if (match && match->mode == MC_MATCH_OFF) match = nullptr;
        if (parts && parts->mode == MC_PARTS_OFF) parts = nullptr;
        return *this;
    }
    bool any() const { return tail || phase || filter || match || parts; }
};

// Steps 1a to 1e of a normalised request as load_ir takes them, beside IrSteps and in its manner.  The checks return the message
// of the first one that fails, null when all pass; no engine and no HIP call.  The tail's own checks (tail_check,
// tail_check_frames) stay with the source, which knows where among its own they belong.
struct StepPlan {
    TailStep tail{};
    PhaseStep phase{};
    FilterStep filter{};
    MatchStep match;
    PartsStep parts{};
    uint64_t G = 0, Gm = 0;  // limits(): the filter's and the target's frames at the session's rate
    bool tailed = false, phased = false, filtered = false, matched = false, parted = false;

    // the structs of the parts, the match, the filter and the phase, in that order
    static const char* check_structs(const StepRequest& rq) {
        if (rq.parts)
            if (const char* bad = parts_check(rq.parts)) return bad;
        if (rq.match)
            if (const char* bad = match_check(rq.match)) return bad;
        if (rq.filter)
            if (const char* bad = filter_check(rq.filter)) return bad;
        return rq.phase ? phase_check(rq.phase) : nullptr;
    }
    // the checked tail over F frames at the session's rate; the frames it hands on
    uint64_t plan_tail(const mc_ir_tail& t, uint32_t session_rate, uint64_t F) {
        tail = tail_step(t, session_rate, F), tailed = true;
        return tail.plan.Fp;
    }
    // the limits of the steps that are on, over the F frames that reach them: the phase's, the filter's, the match's over what the
    // filter hands on, the parts' over what the match hands on
    const char* limits(const StepRequest& rq, uint64_t F, uint32_t session_rate) {
        if (rq.phase)
            if (const char* bad = phase_check_frames(rq.phase, F)) return bad;
        if (rq.filter)
            if (const char* bad = filter_check_load(rq.filter, session_rate, F, rq.filter_frames, &G)) return bad;
        const uint64_t Ff = rq.filter && F ? filter_step(*rq.filter, F, G).Fo : F;
        if (rq.match)
            if (const char* bad = match_check_load(rq.match, session_rate, Ff, rq.target_frames, &Gm)) return bad;
        return rq.parts ? parts_check_frames(rq.parts, rq.match && F ? match_step(*rq.match, session_rate, Ff, Gm).Fo : Ff) : nullptr;
    }
    // the second IRs' frames: the filter's, and the target's when the match has one
    static const char* pointers(const StepRequest& rq) {
        if (rq.filter && !rq.filter_lr) return "null filter_lr";
        return rq.match && rq.match->mode == MC_MATCH_TARGET && !rq.target_lr ? "null target_lr" : nullptr;
    }
    // the three spectral steps and the parts over the F frames that reach them, after limits(); a second IR's rate 0 is the session's
    void plan(const StepRequest& rq, uint64_t F, uint32_t session_rate) {
        phased = rq.phase, filtered = rq.filter, matched = rq.match, parted = rq.parts;
        if (rq.phase) phase = phase_step(*rq.phase, F);
        if (rq.filter) filter = filter_step(*rq.filter, F, G), filter.second = second_ir(rq.filter_lr, rq.filter_frames, rq.filter->rate, session_rate);
        if (rq.match && F) match = match_step(*rq.match, session_rate, rq.filter ? filter.Fo : F, Gm);
        if (rq.match) match.second = second_ir(rq.target_lr, rq.target_frames, rq.match->rate, session_rate);
        if (rq.parts && F) parts = parts_step(*rq.parts, rq.match ? match.Fo : rq.filter ? filter.Fo : F);
    }
    void into(IrLoad& ld) const {
        ld.tail = tailed ? &tail : nullptr;
        ld.phase = phased ? &phase : nullptr;
        ld.filter = filtered ? &filter : nullptr;
        ld.match = matched ? &match : nullptr;
        ld.parts = parted ? &parts : nullptr;
    }
};

// mc_load_ir_tail, _phase, _filter, _match and _parts behind their switches: a file's frames through the steps of rq, of which one is on.
// All before the engine and before any HIP call: the structs of the parts, the match, the filter and the phase; with a tail the tail, the
// rates, the frames and F', the steps' limits over F', then damp, eq and shape; without one damp, eq and shape as in
// mc_load_ir_damped, the rates unless both are 0, the frames and the steps' limits; then the second IRs' pointers.
int load_file_steps(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate, uint32_t session_rate,
                    const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const StepRequest& rq) {
    if (const char* bad = StepPlan::check_structs(rq)) return fail(MC_ERR_ARG, "%s", bad);
    const auto rates = [&](const char* why) -> int {
        for (int k = 0; k < 2; k++) {
            const uint32_t r = k ? ir_rate : session_rate;
            if (r < RS_MIN_RATE || r > RS_MAX_RATE)
                return fail(MC_ERR_ARG, "%s %u outside [%u, %u] (%s)", k ? "ir_rate" : "session_rate", r, RS_MIN_RATE, RS_MAX_RATE, why);
        }
        return MC_OK;
    };
    // the frames at the session's rate, once the rates and the frames are good
    const auto converted = [&] { return ir_rate != session_rate ? rs_out_frames(rs_geom(ir_rate, session_rate), frames) : frames; };
    IrSteps steps;
    StepPlan plan;
    uint64_t F = 0;
    if (rq.tail) {
        if (const char* bad = tail_check(rq.tail, session_rate)) return fail(MC_ERR_ARG, "%s", bad);
        if (const int rc = rates("the tail step needs the session's rate")) return rc;
        if (frames > (1ull << 40)) return fail(MC_ERR_ARG, "IR of %llu frames", (unsigned long long)frames);
        F = converted();
        if (const char* bad = tail_check_frames(rq.tail, F)) return fail(MC_ERR_ARG, "%s", bad);
        F = plan.plan_tail(*rq.tail, session_rate, F);
        if (const char* bad = plan.limits(rq, F, session_rate)) return fail(MC_ERR_ARG, "%s", bad);
        if (const char* bad = resolve_steps(shape, eq, damp, ir_rate, session_rate, &steps)) return fail(MC_ERR_ARG, "%s", bad);
    } else {
        if (const char* bad = resolve_steps(shape, eq, damp, ir_rate, session_rate, &steps)) return fail(MC_ERR_ARG, "%s", bad);
        if (ir_rate || session_rate)  // (0, 0 without a tail: the frames are at the session's rate)
            if (const int rc = rates("both rates 0 = no conversion")) return rc;
        if (frames > (1ull << 40)) return fail(MC_ERR_ARG, "IR of %llu frames", (unsigned long long)frames);
        F = converted();
        if (const char* bad = plan.limits(rq, F, session_rate)) return fail(MC_ERR_ARG, "%s", bad);
    }
    if (const char* bad = StepPlan::pointers(rq)) return fail(MC_ERR_ARG, "%s", bad);
    plan.plan(rq, F, session_rate);
    const uint32_t rs[2] = {ir_rate, session_rate};
    IrLoad ld;
    ld.lr = lr, ld.frames = frames, ld.rs = ir_rate != session_rate ? rs : nullptr;
    plan.into(ld);
    steps.into(ld);
    return load_ir(e, idx, nframes, ld);
}

// mc_load_ir_sweep_tail, _phase, _filter, _match and _parts behind their switches, as load_file_steps: the structs of the parts, the match, the filter
// and the phase, the tail, then everything mc_load_ir_sweep checks in its order with F' and the steps' limits after the lengths,
// the recording, then the second IRs' pointers.
int load_sweep_steps(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, const mc_sweep* sweep, int64_t offset,
                     uint64_t ir_frames, const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const StepRequest& rq) {
    if (const char* bad = StepPlan::check_structs(rq)) return fail(MC_ERR_ARG, "%s", bad);
    if (rq.tail)
        if (const char* bad = tail_check(rq.tail, sweep ? sweep->rate : 0)) return fail(MC_ERR_ARG, "%s", bad);
    if (const char* bad = swp_check(sweep)) return fail(MC_ERR_ARG, "%s", bad);
    if (const char* bad = swp_check_load(sweep, frames, ir_frames, offset)) return fail(MC_ERR_ARG, "%s", bad);
    if (rq.tail)
        if (const char* bad = tail_check_frames(rq.tail, ir_frames)) return fail(MC_ERR_ARG, "%s", bad);
    StepPlan plan;
    const uint64_t F = rq.tail ? plan.plan_tail(*rq.tail, sweep->rate, ir_frames) : ir_frames;
    if (const char* bad = plan.limits(rq, F, sweep->rate)) return fail(MC_ERR_ARG, "%s", bad);
    IrSteps steps;
    if (const char* bad = resolve_steps(shape, eq, damp, sweep->rate, sweep->rate, &steps)) return fail(MC_ERR_ARG, "%s", bad);
    if (!lr) return fail(MC_ERR_ARG, "null lr");
    if (const char* bad = StepPlan::pointers(rq)) return fail(MC_ERR_ARG, "%s", bad);
    plan.plan(rq, F, sweep->rate);
    const SweepSource src{swp_plan(*sweep), lr, frames, ir_frames, offset};
    IrLoad ld;
    ld.swp = &src, ld.frames = ir_frames;
    plan.into(ld);
    steps.into(ld);
    return load_ir(e, idx, nframes, ld);
}
}  // namespace

extern "C" {

int mc_load_ir(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes) {
    IrLoad ld;
    ld.lr = lr, ld.frames = frames;
    return load_ir(e, idx, nframes, ld);
}

int mc_load_ir_resampled(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate,
                         uint32_t session_rate) {
    // rates are checked before any HIP call: a refused load leaves the engine as it was
    for (uint32_t r : {ir_rate, session_rate})
        if (r < RS_MIN_RATE || r > RS_MAX_RATE) return fail(MC_ERR_ARG, "sample rate %u outside [%u, %u]", r, RS_MIN_RATE, RS_MAX_RATE);
    if (frames > (1ull << 40)) return fail(MC_ERR_ARG, "IR of %llu frames", (unsigned long long)frames);
    if (ir_rate == session_rate) return mc_load_ir(e, idx, lr, frames, nframes);
    const uint32_t rs[2] = {ir_rate, session_rate};
    IrLoad ld;
    ld.lr = lr, ld.frames = frames, ld.rs = rs;
    return load_ir(e, idx, nframes, ld);
}

void mc_default_ir_shape(mc_ir_shape* s) {
    if (!s) return;
    std::memset(s, 0, sizeof(*s));
    s->struct_size = (uint32_t)sizeof(*s);
    s->target = 1.f;
}

int mc_load_ir_shaped(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate,
                      uint32_t session_rate, const mc_ir_shape* shape) {
    // the shape and the rates are checked before the pointers and before any HIP call: a refused load leaves the engine as it was
    if (const char* bad = ish_check(shape)) return fail(MC_ERR_ARG, "%s", bad);
    const bool convert = ir_rate || session_rate;  // (0, 0: the frames are at the session's rate)
    if (convert)
        for (int k = 0; k < 2; k++) {
            const uint32_t r = k ? session_rate : ir_rate;
            if (r < RS_MIN_RATE || r > RS_MAX_RATE)
                return fail(MC_ERR_ARG, "%s %u outside [%u, %u] (both rates 0 = no conversion)", k ? "session_rate" : "ir_rate", r, RS_MIN_RATE, RS_MAX_RATE);
        }
    if (frames > (1ull << 40)) return fail(MC_ERR_ARG, "IR of %llu frames", (unsigned long long)frames);
    if (ish_is_off(*shape))
        return convert ? mc_load_ir_resampled(e, idx, lr, frames, nframes, ir_rate, session_rate) : mc_load_ir(e, idx, lr, frames, nframes);
    const uint32_t rs[2] = {ir_rate, session_rate};
    IrLoad ld;
    ld.lr = lr, ld.frames = frames, ld.rs = ir_rate != session_rate ? rs : nullptr;  // (0, 0 are equal)
    ld.shape = shape;
    return load_ir(e, idx, nframes, ld);
}

void mc_default_ir_eq(mc_ir_eq* eq) {
    if (!eq) return;
    std::memset(eq, 0, sizeof(*eq));
    eq->struct_size = (uint32_t)sizeof(*eq);
    for (mc_eq_band& b : eq->band) b = mc_eq_band{MC_EQ_OFF, 1000.f, 0.f, 0.70710678f};
}

int mc_load_ir_eq(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate, uint32_t session_rate,
                  const mc_ir_shape* shape, const mc_ir_eq* eq) {
    // as in mc_load_ir_shaped, everything is checked before the pointers and before any HIP call
    int on = 0;
    if (const char* bad = ieq_check(eq, ir_rate, session_rate, &on)) return fail(MC_ERR_ARG, "%s", bad);
    mc_ir_shape off;
    mc_default_ir_shape(&off);
    if (!shape) shape = &off;
    if (!on) return mc_load_ir_shaped(e, idx, lr, frames, nframes, ir_rate, session_rate, shape);
    if (const char* bad = ish_check(shape)) return fail(MC_ERR_ARG, "%s", bad);
    if (frames > (1ull << 40)) return fail(MC_ERR_ARG, "IR of %llu frames", (unsigned long long)frames);
    const IeqCascade cs = ieq_cascade(*eq, session_rate);
    const uint32_t rs[2] = {ir_rate, session_rate};
    IrLoad ld;
    ld.lr = lr, ld.frames = frames, ld.rs = ir_rate != session_rate ? rs : nullptr;
    ld.shape = shape, ld.eq = &cs;
    return load_ir(e, idx, nframes, ld);
}

int mc_ir_eq_response(const mc_ir_eq* eq, uint32_t rate, const double* hz, uint32_t n, double* db) {
    int on = 0;
    if (const char* bad = ieq_check(eq, rate, rate, &on)) return fail(MC_ERR_ARG, "%s", bad);
    if (n && (!hz || !db)) return fail(MC_ERR_ARG, "null argument");
    if (rate < RS_MIN_RATE || rate > RS_MAX_RATE) return fail(MC_ERR_ARG, "rate %u outside [%u, %u]", rate, RS_MIN_RATE, RS_MAX_RATE);
    const IeqCascade cs = ieq_cascade(*eq, rate);
    for (uint32_t i = 0; i < n; i++) db[i] = ieq_response_db(cs, rate, hz[i]);
    return MC_OK;
}

void mc_default_ir_damp(mc_ir_damp* d) {
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    d->struct_size = (uint32_t)sizeof(*d);
    d->xover_hz[0] = 250.f, d->xover_hz[1] = 2000.f, d->xover_hz[2] = 8000.f;
}

int mc_load_ir_damped(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate, uint32_t session_rate,
                      const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp) {
    mc_ir_eq noeq;
    mc_default_ir_eq(&noeq);
    if (!eq) eq = &noeq;
    if (!damp || !damp->n_xovers) return mc_load_ir_eq(e, idx, lr, frames, nframes, ir_rate, session_rate, shape, eq);
    // as in mc_load_ir_eq, everything is checked before the pointers and before any HIP call
    IrSteps steps;
    if (const char* bad = resolve_steps(shape, eq, damp, ir_rate, session_rate, &steps)) return fail(MC_ERR_ARG, "%s", bad);
    if (frames > (1ull << 40)) return fail(MC_ERR_ARG, "IR of %llu frames", (unsigned long long)frames);
    const uint32_t rs[2] = {ir_rate, session_rate};
    IrLoad ld;
    ld.lr = lr, ld.frames = frames, ld.rs = ir_rate != session_rate ? rs : nullptr;
    steps.into(ld);
    return load_ir(e, idx, nframes, ld);
}

void mc_default_ir_synth(mc_ir_synth* s) {
    if (!s) return;
    std::memset(s, 0, sizeof(*s));
    s->struct_size = (uint32_t)sizeof(*s);
    s->late_gain = s->early_gain = s->width = 1.f;
}

int mc_synth_ir(mc_engine* e, uint64_t idx, uint64_t nframes, const mc_ir_synth* synth, const mc_ir_shape* shape, const mc_ir_eq* eq,
                const mc_ir_damp* damp) {
    // the struct first, then damp, eq and shape as in mc_load_ir_damped, all before the engine and before any HIP call
    if (const char* bad = syn_check(synth)) return fail(MC_ERR_ARG, "%s", bad);
    IrSteps steps;
    if (const char* bad = resolve_steps(shape, eq, damp, synth->rate, synth->rate, &steps)) return fail(MC_ERR_ARG, "%s", bad);
    const SynPlan syn = syn_plan(*synth);
    IrLoad ld;
    ld.syn = &syn, ld.frames = synth->frames;
    steps.into(ld);
    return load_ir(e, idx, nframes, ld);
}

void mc_default_ir_room(mc_ir_room* r) {
    if (!r) return;
    std::memset(r, 0, sizeof(*r));
    r->struct_size = (uint32_t)sizeof(*r);
    r->size_m[0] = 5.f, r->size_m[1] = 4.f, r->size_m[2] = 3.f;
    r->source_m[0] = 1.f, r->source_m[1] = 1.5f, r->source_m[2] = 1.2f;
    r->receiver_m[0] = 3.5f, r->receiver_m[1] = 2.f, r->receiver_m[2] = 1.5f;
    for (float& b : r->beta) b = 0.9f;
    r->spacing_m = 0.2f;
    r->speed = 343.f;
    r->gain = 1.f;
}

void mc_default_ir_room_mics(mc_ir_room_mics* m) {
    if (!m) return;
    std::memset(m, 0, sizeof(*m));
    m->struct_size = (uint32_t)sizeof(*m);
    m->mic_pattern[0] = m->mic_pattern[1] = m->src_pattern = 1.f;
}

int mc_synth_ir_room(mc_engine* e, uint64_t idx, uint64_t nframes, const mc_ir_synth* synth, const mc_ir_room* room, const mc_ir_shape* shape,
                     const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail) {
    return mc_synth_ir_room_mics(e, idx, nframes, synth, room, nullptr, shape, eq, damp, tail);
}

int mc_synth_ir_room_mics(mc_engine* e, uint64_t idx, uint64_t nframes, const mc_ir_synth* synth, const mc_ir_room* room, const mc_ir_room_mics* mics,
                          const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail) {
    return mc_synth_ir_room_bands(e, idx, nframes, synth, room, mics, nullptr, shape, eq, damp, tail);
}

void mc_default_ir_room_bands(mc_ir_room_bands* b) {
    if (!b) return;
    std::memset(b, 0, sizeof(*b));
    b->struct_size = (uint32_t)sizeof(*b);
    for (auto& band : b->beta)
        for (float& v : band) v = 0.9f;
}

int mc_synth_ir_room_bands(mc_engine* e, uint64_t idx, uint64_t nframes, const mc_ir_synth* synth, const mc_ir_room* room, const mc_ir_room_mics* mics,
                           const mc_ir_room_bands* bands, const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail) {
    return mc_synth_ir_room_head(e, idx, nframes, synth, room, mics, bands, nullptr, shape, eq, damp, tail);
}

void mc_default_ir_room_head(mc_ir_room_head* h) {
    if (!h) return;
    std::memset(h, 0, sizeof(*h));
    h->struct_size = (uint32_t)sizeof(*h);
    h->radius_m = 0.0875f;
    h->ear_deg = 90.f;
    h->shadow = 1.f;
}

int mc_synth_ir_room_head(mc_engine* e, uint64_t idx, uint64_t nframes, const mc_ir_synth* synth, const mc_ir_room* room, const mc_ir_room_mics* mics,
                          const mc_ir_room_bands* bands, const mc_ir_room_head* head, const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp,
                          const mc_ir_tail* tail) {
    const bool tailed = tail && tail->mode != MC_TAIL_OFF;
    if (!room && !mics && !bands && !head && !tailed) return mc_synth_ir(e, idx, nframes, synth, shape, eq, damp);
    // synth, then the room, its microphones, its bands and its head, then the tail with F' after F, then damp, eq and shape as in
    // mc_synth_ir, all before the engine and before any HIP call
    if (const char* bad = syn_check(synth)) return fail(MC_ERR_ARG, "%s", bad);
    const uint32_t rate = synth->rate;
    const uint64_t F = synth->frames;
    if (mics && !room) return fail(MC_ERR_ARG, "the microphones need a room");
    if (room)
        if (const char* bad = room_check(room, rate, F)) return fail(MC_ERR_ARG, "%s", bad);
    if (mics)
        if (const char* bad = room_mics_check(mics)) return fail(MC_ERR_ARG, "%s", bad);
    if (bands && !room) return fail(MC_ERR_ARG, "the bands need a room");
    if (bands)
        if (const char* bad = room_bands_check(bands, rate)) return fail(MC_ERR_ARG, "%s", bad);
    if (head && !room) return fail(MC_ERR_ARG, "the head needs a room");
    if (head)
        if (const char* bad = room_head_check(head, *room, mics, rate, F)) return fail(MC_ERR_ARG, "%s", bad);
    if (tailed) {
        if (const char* bad = tail_check(tail, rate)) return fail(MC_ERR_ARG, "%s", bad);
        if (rate < RS_MIN_RATE || rate > RS_MAX_RATE)
            return fail(MC_ERR_ARG, "rate %u outside [%u, %u] (the tail step needs the session's rate)", rate, RS_MIN_RATE, RS_MAX_RATE);
        if (const char* bad = tail_check_frames(tail, F)) return fail(MC_ERR_ARG, "%s", bad);
    }
    IrSteps steps;
    if (const char* bad = resolve_steps(shape, eq, damp, rate, rate, &steps)) return fail(MC_ERR_ARG, "%s", bad);
    const SynPlan syn = syn_plan(*synth);
    TailStep step{};
    if (tailed) step = tail_step(*tail, rate, F);
    RoomStep rstep{};
    if (room) rstep.plan = room_plan(*room, rate, F);
    if (head) room_plan_head(rstep.plan, *room, *head, rstep.head);
    if (mics) room_plan_mics(rstep.plan, *mics);
    if (bands) rstep.bands = room_bands_plan(rstep.plan, *room, *bands, rate), rstep.banded = true;
    IrLoad ld;
    ld.syn = &syn, ld.frames = F;
    ld.room = room ? &rstep : nullptr;
    ld.tail = tailed ? &step : nullptr;
    steps.into(ld);
    return load_ir(e, idx, nframes, ld);
}

int mc_ir_room_info(const mc_engine* e, uint64_t idx, double out[8]) { return ir_fact(e, idx, FACT_ROOM, 8, "was not loaded with a room", out); }

int mc_ir_room_plan(const mc_ir_room* room, uint32_t rate, uint64_t frames, double out[8]) {
    if (frames < 1 || frames > SYN_MAX_FRAMES)
        return fail(MC_ERR_ARG, "frames %llu outside [1, %llu]", (unsigned long long)frames, (unsigned long long)SYN_MAX_FRAMES);
    if (const char* bad = room_check(room, rate, frames)) return fail(MC_ERR_ARG, "%s", bad);
    if (!out) return fail(MC_ERR_ARG, "null out");
    room_report(*room, rate, frames, out);
    return MC_OK;
}

int mc_ir_room_mics_plan(const mc_ir_room* room, const mc_ir_room_mics* mics, uint32_t rate, uint64_t frames, double out[8]) {
    if (frames < 1 || frames > SYN_MAX_FRAMES)
        return fail(MC_ERR_ARG, "frames %llu outside [1, %llu]", (unsigned long long)frames, (unsigned long long)SYN_MAX_FRAMES);
    if (const char* bad = room_check(room, rate, frames)) return fail(MC_ERR_ARG, "%s", bad);
    if (const char* bad = room_mics_check(mics)) return fail(MC_ERR_ARG, "%s", bad);
    if (!out) return fail(MC_ERR_ARG, "null out");
    RoomPlan p = room_plan(*room, rate, frames);
    room_plan_mics(p, *mics);
    room_mics_report(p, out);
    return MC_OK;
}

int mc_ir_room_mics_info(const mc_engine* e, uint64_t idx, double out[8]) {
    return ir_fact(e, idx, FACT_ROOM_MICS, 8, "was not loaded with microphones", out);
}

int mc_ir_room_bands_plan(const mc_ir_room* room, const mc_ir_room_bands* bands, uint32_t rate, uint64_t frames, double out[16]) {
    if (frames < 1 || frames > SYN_MAX_FRAMES)
        return fail(MC_ERR_ARG, "frames %llu outside [1, %llu]", (unsigned long long)frames, (unsigned long long)SYN_MAX_FRAMES);
    if (const char* bad = room_check(room, rate, frames)) return fail(MC_ERR_ARG, "%s", bad);
    if (const char* bad = room_bands_check(bands, rate)) return fail(MC_ERR_ARG, "%s", bad);
    if (!out) return fail(MC_ERR_ARG, "null out");
    room_bands_report(*room, *bands, out);
    return MC_OK;
}

int mc_ir_room_bands_info(const mc_engine* e, uint64_t idx, double out[16]) {
    return ir_fact(e, idx, FACT_ROOM_BANDS, 16, "was not loaded with bands", out);
}

int mc_ir_room_head_plan(const mc_ir_room* room, const mc_ir_room_head* head, uint32_t rate, uint64_t frames, double out[12]) {
    if (frames < 1 || frames > SYN_MAX_FRAMES)
        return fail(MC_ERR_ARG, "frames %llu outside [1, %llu]", (unsigned long long)frames, (unsigned long long)SYN_MAX_FRAMES);
    if (const char* bad = room_check(room, rate, frames)) return fail(MC_ERR_ARG, "%s", bad);
    if (const char* bad = room_head_check(head, *room, nullptr, rate, frames)) return fail(MC_ERR_ARG, "%s", bad);
    if (!out) return fail(MC_ERR_ARG, "null out");
    RoomPlan p = room_plan(*room, rate, frames);
    room_plan_head(p, *room, *head, out);
    return MC_OK;
}

int mc_ir_room_head_info(const mc_engine* e, uint64_t idx, double out[12]) {
    return ir_fact(e, idx, FACT_ROOM_HEAD, 12, "was not loaded with a head", out);
}

void mc_default_ir_plate(mc_ir_plate* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->size_m[0] = 2.04f, p->size_m[1] = 0.97f;
    p->thickness_mm = 0.5f;
    p->young_gpa = 200.f, p->density = 7850.f, p->poisson = 0.3f;
    p->driver_m[0] = 0.83f, p->driver_m[1] = 0.41f;
    p->pickup_m[0][0] = 0.31f, p->pickup_m[0][1] = 0.67f;
    p->pickup_m[1][0] = 1.57f, p->pickup_m[1][1] = 0.29f;
    p->low_hz = 20.f;
    p->t60_s[0] = 4.f, p->t60_s[1] = 1.f;
    p->damp_hz = 10000.f;
    p->gain = 1.f;
}

int mc_synth_ir_plate(mc_engine* e, uint64_t idx, uint64_t nframes, const mc_ir_synth* synth, const mc_ir_plate* plate, const mc_ir_shape* shape,
                      const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail) {
    if (!plate) return mc_synth_ir_room(e, idx, nframes, synth, nullptr, shape, eq, damp, tail);
    // synth, then the plate, then the tail with F' after F, then damp, eq and shape as in mc_synth_ir_room, all before the engine
    // and before any HIP call
    if (const char* bad = syn_check(synth)) return fail(MC_ERR_ARG, "%s", bad);
    const uint32_t rate = synth->rate;
    const uint64_t F = synth->frames;
    PlateStep pstep;
    if (const char* bad = plate_check(plate, rate, F, &pstep.plan)) return fail(MC_ERR_ARG, "%s", bad);
    const bool tailed = tail && tail->mode != MC_TAIL_OFF;
    if (tailed) {
        if (const char* bad = tail_check(tail, rate)) return fail(MC_ERR_ARG, "%s", bad);
        if (const char* bad = tail_check_frames(tail, F)) return fail(MC_ERR_ARG, "%s", bad);
    }
    IrSteps steps;
    if (const char* bad = resolve_steps(shape, eq, damp, rate, rate, &steps)) return fail(MC_ERR_ARG, "%s", bad);
    const SynPlan syn = syn_plan(*synth);
    TailStep step{};
    if (tailed) step = tail_step(*tail, rate, F);
    IrLoad ld;
    ld.syn = &syn, ld.frames = F;
    ld.plate = &pstep;
    ld.tail = tailed ? &step : nullptr;
    steps.into(ld);
    return load_ir(e, idx, nframes, ld);
}

int mc_ir_plate_plan(const mc_ir_plate* plate, uint32_t rate, uint64_t frames, double out[8]) {
    if (frames < 1 || frames > SYN_MAX_FRAMES)
        return fail(MC_ERR_ARG, "frames %llu outside [1, %llu]", (unsigned long long)frames, (unsigned long long)SYN_MAX_FRAMES);
    PlatePlan p;
    if (const char* bad = plate_check(plate, rate, frames, &p)) return fail(MC_ERR_ARG, "%s", bad);
    if (!out) return fail(MC_ERR_ARG, "null out");
    const double v[8] = {(double)p.M, p.lo, p.hi, p.kappa, p.density, p.t60_lo, p.t60_hi, (double)p.E * (double)p.M};
    std::copy(v, v + 8, out);
    return MC_OK;
}

int mc_ir_plate_modes(const mc_ir_plate* plate, uint32_t rate, uint64_t first, uint64_t count, double* rows) {
    PlatePlan p;
    if (const char* bad = plate_check(plate, rate, 0, &p)) return fail(MC_ERR_ARG, "%s", bad);
    if (first > p.M || count > p.M - first)
        return fail(MC_ERR_ARG, "rows %llu to %llu of a table of %llu", (unsigned long long)first, (unsigned long long)(first + count), (unsigned long long)p.M);
    if (count && !rows) return fail(MC_ERR_ARG, "null rows");
    static_assert(sizeof(PlateMode) == 6 * sizeof(double), "a row of the mode table is six doubles");
    if (count) std::memcpy(rows, p.modes.data() + first, sizeof(PlateMode) * count);
    return MC_OK;
}

int mc_ir_plate_info(const mc_engine* e, uint64_t idx, double out[8]) { return ir_fact(e, idx, FACT_PLATE, 8, "was not loaded with a plate", out); }

void mc_default_ir_spring(mc_ir_spring* s) {
    if (!s) return;
    std::memset(s, 0, sizeof(*s));
    s->struct_size = (uint32_t)sizeof(*s);
    s->sections = 100;
    s->transition_hz = 4300.f;
    s->dispersion = 0.62f;
    s->delay_ms[0] = 66.f, s->delay_ms[1] = 82.f;
    s->t60_s = 2.5f;
    s->damping = 0.2f;
    s->lowpass_order = 8;
    s->high_gain = 0.1f;
    s->high_sections = 200;
    s->high_dispersion = -0.6f;
    s->high_delay = 0.5f;
    s->high_t60_s = 1.f;
    s->stereo = 0.03f;
    s->gain = 1.f;
}

int mc_synth_ir_spring(mc_engine* e, uint64_t idx, uint64_t nframes, const mc_ir_synth* synth, const mc_ir_spring* spring, const mc_ir_shape* shape,
                       const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail) {
    if (!spring) return mc_synth_ir_room(e, idx, nframes, synth, nullptr, shape, eq, damp, tail);
    // synth, then the spring, then the tail with F' after F, then damp, eq and shape as in mc_synth_ir_plate, all before the engine
    // and before any HIP call
    if (const char* bad = syn_check(synth)) return fail(MC_ERR_ARG, "%s", bad);
    const uint32_t rate = synth->rate;
    const uint64_t F = synth->frames;
    SpringStep sstep;
    if (const char* bad = spring_check(spring, rate, F, &sstep.plan)) return fail(MC_ERR_ARG, "%s", bad);
    const bool tailed = tail && tail->mode != MC_TAIL_OFF;
    if (tailed) {
        if (const char* bad = tail_check(tail, rate)) return fail(MC_ERR_ARG, "%s", bad);
        if (const char* bad = tail_check_frames(tail, F)) return fail(MC_ERR_ARG, "%s", bad);
    }
    IrSteps steps;
    if (const char* bad = resolve_steps(shape, eq, damp, rate, rate, &steps)) return fail(MC_ERR_ARG, "%s", bad);
    const SynPlan syn = syn_plan(*synth);
    TailStep step{};
    if (tailed) step = tail_step(*tail, rate, F);
    IrLoad ld;
    ld.syn = &syn, ld.frames = F;
    ld.spring = &sstep;
    ld.tail = tailed ? &step : nullptr;
    steps.into(ld);
    return load_ir(e, idx, nframes, ld);
}

int mc_ir_spring_plan(const mc_ir_spring* spring, uint32_t rate, uint64_t frames, double out[24]) {
    if (frames < 1 || frames > SYN_MAX_FRAMES)
        return fail(MC_ERR_ARG, "frames %llu outside [1, %llu]", (unsigned long long)frames, (unsigned long long)SYN_MAX_FRAMES);
    SpringPlan p;
    if (const char* bad = spring_check(spring, rate, frames, &p)) return fail(MC_ERR_ARG, "%s", bad);
    if (!out) return fail(MC_ERR_ARG, "null out");
    spring_numbers(p, out);
    return MC_OK;
}

int mc_ir_spring_response(const mc_ir_spring* spring, uint32_t rate, const double* hz, uint32_t n, double* out_re_im) {
    SpringPlan p;
    if (const char* bad = spring_check(spring, rate, 0, &p)) return fail(MC_ERR_ARG, "%s", bad);
    if (n && (!hz || !out_re_im)) return fail(MC_ERR_ARG, "null hz or out_re_im");
    for (uint32_t i = 0; i < n; i++) {
        if (!std::isfinite(hz[i])) return fail(MC_ERR_ARG, "hz[%u] is not finite", i);
        spring_response(p.k, rate, hz[i], out_re_im + 4 * (size_t)i);
    }
    return MC_OK;
}

int mc_ir_spring_info(const mc_engine* e, uint64_t idx, double out[24]) { return ir_fact(e, idx, FACT_SPRING, 24, "was not loaded with a spring", out); }

int mc_ir_synth_info(const mc_engine* e, uint64_t idx, double out[4]) { return ir_fact(e, idx, FACT_SYNTH, 4, "was not synthesised", out); }

void mc_default_sweep(mc_sweep* sw) {
    if (!sw) return;
    std::memset(sw, 0, sizeof(*sw));
    sw->struct_size = (uint32_t)sizeof(*sw);
    sw->rate = 44100;
    sw->f1_hz = 20.f;
    sw->f2_hz = 20000.f;
    sw->amplitude = 0.5f;
}

int mc_sweep_generate(const mc_sweep* sw, float* out, uint64_t first, uint64_t count) {
    if (const char* bad = swp_check(sw)) return fail(MC_ERR_ARG, "%s", bad);
    if (first > sw->frames || count > sw->frames - first)
        return fail(MC_ERR_ARG, "first %llu + count %llu above frames %llu", (unsigned long long)first, (unsigned long long)count,
                    (unsigned long long)sw->frames);
    if (!out) return fail(MC_ERR_ARG, "null out");
    const SweepPlan p = swp_plan(*sw);
    for (uint64_t i = 0; i < count; i++) out[i] = (float)swp_s64(p, first + i);
    return MC_OK;
}

int mc_load_ir_sweep(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, const mc_sweep* sweep, int64_t offset,
                     uint64_t ir_frames, const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp) {
    // the sweep first, then the lengths, then damp, eq and shape as in mc_load_ir_damped, all before the engine and before any HIP call
    if (const char* bad = swp_check(sweep)) return fail(MC_ERR_ARG, "%s", bad);
    if (const char* bad = swp_check_load(sweep, frames, ir_frames, offset)) return fail(MC_ERR_ARG, "%s", bad);
    IrSteps steps;
    if (const char* bad = resolve_steps(shape, eq, damp, sweep->rate, sweep->rate, &steps)) return fail(MC_ERR_ARG, "%s", bad);
    if (!lr) return fail(MC_ERR_ARG, "null lr");
    const SweepSource src{swp_plan(*sweep), lr, frames, ir_frames, offset};
    IrLoad ld;
    ld.swp = &src, ld.frames = ir_frames;
    steps.into(ld);
    return load_ir(e, idx, nframes, ld);
}

int mc_ir_sweep_info(const mc_engine* e, uint64_t idx, double out[4]) { return ir_fact(e, idx, FACT_SWEEP, 4, "was not loaded from a sweep", out); }

int mc_ir_damp_info(const mc_engine* e, uint64_t idx, double out[4]) { return ir_fact(e, idx, FACT_DAMP, 4, "was not loaded with damping", out); }

int mc_ir_damp_response(const mc_ir_damp* d, uint32_t rate, uint64_t tap, const double* hz, uint32_t n, double* db) {
    if (!d) return fail(MC_ERR_ARG, "null damp");
    if (d->n_xovers)
        if (const char* bad = damp_check(d, rate, rate)) return fail(MC_ERR_ARG, "%s", bad);
    if (n && (!hz || !db)) return fail(MC_ERR_ARG, "null argument");
    if (!d->n_xovers) {
        for (uint32_t i = 0; i < n; i++) db[i] = 0.0;
        return MC_OK;
    }
    const DampPlan pl = damp_plan(*d, rate);
    for (uint32_t i = 0; i < n; i++) db[i] = damp_response_db(pl, rate, tap, hz[i]);
    return MC_OK;
}

void mc_default_decay_query(mc_decay_query* q) {
    if (!q) return;
    std::memset(q, 0, sizeof(*q));
    q->struct_size = (uint32_t)sizeof(*q);
    q->rate = 44100;
    q->q = 1.41421356f;
    q->onset_db = -20.f;
}

int mc_ir_decay(mc_engine* e, uint64_t idx, const mc_decay_query* q, double* rows, double* curve, uint64_t info[2]) {
    // the query, the pointers and the index are checked in this order before any HIP call
    if (const char* bad = dec_check(q)) return fail(MC_ERR_ARG, "%s", bad);
    if (!e) return fail(MC_ERR_ARG, "null engine");
    if (!rows) return fail(MC_ERR_ARG, "null rows");
    if (q->curve_points && !curve) return fail(MC_ERR_ARG, "null curve with curve_points %u", q->curve_points);
    if (!info) return fail(MC_ERR_ARG, "null info");
    return measure(e, idx, "decay", [&](const float2* d_x, uint64_t n) { return dec_measure(e->stream, d_x, n, *q, rows, curve, info); });
}

void mc_default_floor_query(mc_floor_query* q) {
    if (!q) return;
    std::memset(q, 0, sizeof(*q));
    q->struct_size = (uint32_t)sizeof(*q);
    q->rate = 44100;
    q->xover_hz[0] = 250.f, q->xover_hz[1] = 2000.f, q->xover_hz[2] = 8000.f;
    q->onset_db = -20.f;
    q->tail_fraction = 0.1f;
    q->margin_db = 10.f;
    q->span_db = 20.f;
    q->per_decade = 5;
    q->rounds = 5;
}

int mc_ir_floor(mc_engine* e, uint64_t idx, const mc_floor_query* q, double* rows, uint64_t info[2]) {
    // the query, the pointers and the index are checked in this order before any HIP call
    if (const char* bad = flr_check(q)) return fail(MC_ERR_ARG, "%s", bad);
    if (!e) return fail(MC_ERR_ARG, "null engine");
    if (!rows) return fail(MC_ERR_ARG, "null rows");
    if (!info) return fail(MC_ERR_ARG, "null info");
    return measure(e, idx, "floor", [&](const float2* d_x, uint64_t n) { return flr_measure(e->stream, d_x, n, *q, rows, info); });
}

int mc_ir_tail_from_floor(const mc_floor_query* q, const double* rows, const uint64_t info[2], uint64_t first, mc_ir_tail* tail) {
    if (const char* bad = flr_check(q)) return fail(MC_ERR_ARG, "%s", bad);
    if (!rows) return fail(MC_ERR_ARG, "null rows");
    if (!info) return fail(MC_ERR_ARG, "null info");
    if (!tail) return fail(MC_ERR_ARG, "null tail");
    if (tail->struct_size != sizeof(mc_ir_tail)) return fail(MC_ERR_ARG, "mc_ir_tail struct_size mismatch");
    flr_to_tail(*q, rows, info, first, tail);
    return MC_OK;
}

void mc_default_density_query(mc_density_query* q) {
    if (!q) return;
    std::memset(q, 0, sizeof(*q));
    q->struct_size = (uint32_t)sizeof(*q);
    q->rate = 44100;
    q->onset_db = -20.f;
    q->threshold = 1.f;
}

int mc_ir_density(mc_engine* e, uint64_t idx, const mc_density_query* q, double* rows, double* profile, uint64_t info[3]) {
    // the query, the pointers, the index and the work bounds are checked in this order before any HIP call
    if (const char* bad = den_check(q)) return fail(MC_ERR_ARG, "%s", bad);
    if (!e) return fail(MC_ERR_ARG, "null engine");
    if (!rows) return fail(MC_ERR_ARG, "null rows");
    if (!info) return fail(MC_ERR_ARG, "null info");
    return measure(
        e, idx, "density", [&](uint64_t n) { return den_check_work(*q, n); },
        [&](const float2* d_x, uint64_t n) { return den_measure(e->stream, d_x, n, *q, rows, profile, info); });
}

int mc_ir_tail_move_knee(mc_ir_tail* tail, uint32_t band, uint64_t frame) {
    if (!tail) return fail(MC_ERR_ARG, "null tail");
    if (tail->struct_size != sizeof(mc_ir_tail)) return fail(MC_ERR_ARG, "mc_ir_tail struct_size mismatch");
    if (tail->n_xovers > 3 || band > tail->n_xovers) return fail(MC_ERR_ARG, "band %u above n_xovers %u", band, tail->n_xovers);
    if (tail->knee[band] == FLR_LEFT_ALONE) return fail(MC_ERR_ARG, "band %u has no knee to move (it is left alone)", band);
    if (tail->mode != MC_TAIL_EXTEND) return fail(MC_ERR_ARG, "mode %u is not MC_TAIL_EXTEND: only an extended tail has levels to slide", tail->mode);
    den_move_knee(tail, band, frame);
    return MC_OK;
}

void mc_default_iacc_query(mc_iacc_query* q) {
    if (!q) return;
    std::memset(q, 0, sizeof(*q));
    q->struct_size = (uint32_t)sizeof(*q);
    q->rate = 44100;
    q->max_lag = 44;
    q->q = 1.41421356f;
    q->onset_db = -20.f;
}

int mc_ir_iacc(mc_engine* e, uint64_t idx, const mc_iacc_query* q, double* rows, double* curve, uint64_t info[3]) {
    // the query, the pointers, the index and the work bounds are checked in this order before any HIP call
    if (const char* bad = iacc_check(q)) return fail(MC_ERR_ARG, "%s", bad);
    if (!e) return fail(MC_ERR_ARG, "null engine");
    if (!rows) return fail(MC_ERR_ARG, "null rows");
    if (!info) return fail(MC_ERR_ARG, "null info");
    return measure(
        e, idx, "IACC", [&](uint64_t n) { return iacc_check_work(*q, n); },
        [&](const float2* d_x, uint64_t n) { return iacc_measure(e->stream, d_x, n, *q, rows, curve, info); });
}

int mc_ir_tail_width_from_iacc(mc_ir_tail* tail, double rho) {
    if (!tail) return fail(MC_ERR_ARG, "null tail");
    if (tail->struct_size != sizeof(mc_ir_tail)) return fail(MC_ERR_ARG, "mc_ir_tail struct_size mismatch");
    if (!std::isfinite(rho)) return fail(MC_ERR_ARG, "rho %g is not finite", rho);
    tail->width = iacc_width(rho);
    return MC_OK;
}

void mc_default_sti_query(mc_sti_query* q) {
    if (!q) return;
    std::memset(q, 0, sizeof(*q));
    q->struct_size = (uint32_t)sizeof(*q);
    q->rate = 44100;
    q->n_bands = MC_STI_MAX_BANDS;
    q->n_mod = 14;
    // the octaves, IEC 60268-16's modulation frequencies and its weights for male speech
    const float centre[MC_STI_MAX_BANDS] = {125.f, 250.f, 500.f, 1000.f, 2000.f, 4000.f, 8000.f};
    const double alpha[MC_STI_MAX_BANDS] = {0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173};
    const double beta[MC_STI_MAX_BANDS - 1] = {0.085, 0.078, 0.065, 0.011, 0.047, 0.095};
    const float mod[14] = {0.63f, 0.8f, 1.f, 1.25f, 1.6f, 2.f, 2.5f, 3.15f, 4.f, 5.f, 6.3f, 8.f, 10.f, 12.5f};
    std::copy(centre, centre + MC_STI_MAX_BANDS, q->centre_hz);
    std::copy(alpha, alpha + MC_STI_MAX_BANDS, q->alpha);
    std::copy(beta, beta + MC_STI_MAX_BANDS - 1, q->beta);
    std::copy(mod, mod + 14, q->mod_hz);
    q->q = 1.41421356f;
    q->onset_db = -20.f;
}

int mc_ir_sti(mc_engine* e, uint64_t idx, const mc_sti_query* q, double* rows, double* mtf, double sti[3], uint64_t info[2]) {
    // the query, the pointers and the index are checked in this order before any HIP call
    if (const char* bad = sti_check(q)) return fail(MC_ERR_ARG, "%s", bad);
    if (!e) return fail(MC_ERR_ARG, "null engine");
    if (!rows) return fail(MC_ERR_ARG, "null rows");
    if (!mtf) return fail(MC_ERR_ARG, "null mtf");
    if (!sti) return fail(MC_ERR_ARG, "null sti");
    if (!info) return fail(MC_ERR_ARG, "null info");
    return measure(e, idx, "STI", [&](const float2* d_x, uint64_t n) { return sti_measure(e->stream, d_x, n, *q, rows, mtf, sti, info); });
}

void mc_default_response_query(mc_response_query* q) {
    if (!q) return;
    std::memset(q, 0, sizeof(*q));
    q->struct_size = (uint32_t)sizeof(*q);
    q->rate = 44100;
    q->n_win = 1;
    q->onset_db = -20.f;
}

int mc_ir_response(mc_engine* e, uint64_t idx, const mc_response_query* q, const float* hz, const mc_response_window* win, double* resp,
                   double* rows, uint64_t* spans, uint64_t info[2]) {
    // the query, the frequencies, the pointers and the index are checked in this order before any HIP call
    if (const char* bad = rsp_check(q, hz)) return fail(MC_ERR_ARG, "%s", bad);
    if (!hz) return fail(MC_ERR_ARG, "null hz");
    if (!win && q->n_win > 1) return fail(MC_ERR_ARG, "null win with n_win %u", q->n_win);
    if (!resp) return fail(MC_ERR_ARG, "null resp");
    if (!rows) return fail(MC_ERR_ARG, "null rows");
    if (!spans) return fail(MC_ERR_ARG, "null spans");
    if (!info) return fail(MC_ERR_ARG, "null info");
    if (!e) return fail(MC_ERR_ARG, "null engine");
    return measure(e, idx, "response",
                   [&](const float2* d_x, uint64_t n) { return rsp_measure(e->stream, d_x, n, *q, hz, win, resp, rows, spans, info); });
}

int mc_response_grid(double lo_hz, double hi_hz, uint32_t per_octave, float* hz, uint32_t cap) {
    if (!(std::isfinite(lo_hz) && std::isfinite(hi_hz) && lo_hz > 0.0 && lo_hz <= hi_hz))
        return fail(MC_ERR_ARG, "lo_hz %g, hi_hz %g: 0 < lo_hz <= hi_hz is required", lo_hz, hi_hz);
    if (per_octave < 1 || per_octave > 96) return fail(MC_ERR_ARG, "per_octave %u outside [1, 96]", per_octave);
    if (!hz) return fail(MC_ERR_ARG, "null hz");
    const int count = rsp_grid(lo_hz, hi_hz, per_octave, hz, cap);
    if (count < 0) return fail(MC_ERR_ARG, "the grid has more than cap %u frequencies", cap);
    return count;
}

int mc_response_smooth(const float* hz, const double* power, uint32_t n, double octaves, double* out) {
    if (!hz) return fail(MC_ERR_ARG, "null hz");
    if (!power) return fail(MC_ERR_ARG, "null power");
    if (!out) return fail(MC_ERR_ARG, "null out");
    if (!(octaves >= 0.0 && octaves <= 10.0)) return fail(MC_ERR_ARG, "octaves %g outside [0, 10]", octaves);
    for (uint32_t f = 0; f < n; f++)
        if (const double v = (double)hz[f]; !(std::isfinite(v) && v >= 0.0 && (f == 0 || v >= (double)hz[f - 1])))
            return fail(MC_ERR_ARG, "hz[%u] %g: the frequencies must be finite, >= 0 and ascend", f, v);
    rsp_smooth(hz, power, n, octaves, out);
    return MC_OK;
}

void mc_default_ir_tail(mc_ir_tail* t) {
    if (!t) return;
    std::memset(t, 0, sizeof(*t));
    t->struct_size = (uint32_t)sizeof(*t);
    t->mode = MC_TAIL_OFF;
    t->xover_hz[0] = 250.f, t->xover_hz[1] = 2000.f, t->xover_hz[2] = 8000.f;
    t->width = 1.f;
    for (int j = 0; j < 4; j++) t->knee[j] = ~0ull, t->t60[j] = 1;
}

int mc_load_ir_tail(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate, uint32_t session_rate,
                    const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail) {
    StepRequest rq;
    rq.tail = tail;
    if (!rq.normalise().any()) return mc_load_ir_damped(e, idx, lr, frames, nframes, ir_rate, session_rate, shape, eq, damp);
    return load_file_steps(e, idx, lr, frames, nframes, ir_rate, session_rate, shape, eq, damp, rq);
}

int mc_load_ir_sweep_tail(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, const mc_sweep* sweep, int64_t offset,
                          uint64_t ir_frames, const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail) {
    StepRequest rq;
    rq.tail = tail;
    if (!rq.normalise().any()) return mc_load_ir_sweep(e, idx, lr, frames, nframes, sweep, offset, ir_frames, shape, eq, damp);
    return load_sweep_steps(e, idx, lr, frames, nframes, sweep, offset, ir_frames, shape, eq, damp, rq);
}

int mc_ir_tail_info(const mc_engine* e, uint64_t idx, double out[4]) { return ir_fact(e, idx, FACT_TAIL, 4, "was not loaded with a tail step", out); }

void mc_default_ir_phase(mc_ir_phase* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->mode = MC_PHASE_OFF;
    p->floor_db = 120.f;
    p->over_log2 = 3;
}

int mc_ir_phase_plan(const mc_ir_phase* p, uint64_t frames, double out[4]) {
    if (!p) return fail(MC_ERR_ARG, "null phase");
    if (const char* bad = phase_check(p)) return fail(MC_ERR_ARG, "%s", bad);
    if (!frames) return fail(MC_ERR_ARG, "empty IR");
    if (const char* bad = phase_check_frames(p, frames)) return fail(MC_ERR_ARG, "%s", bad);
    if (!out) return fail(MC_ERR_ARG, "null out");
    const PhaseStep s = phase_step(*p, frames);
    out[0] = (double)s.Nfft, out[1] = (double)s.fft.passes, out[2] = (double)phase_device_bytes(s), out[3] = 0.0;
    return MC_OK;
}

int mc_load_ir_phase(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate, uint32_t session_rate,
                     const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail, const mc_ir_phase* phase) {
    StepRequest rq;
    rq.tail = tail, rq.phase = phase;
    if (!rq.normalise().any()) return mc_load_ir_damped(e, idx, lr, frames, nframes, ir_rate, session_rate, shape, eq, damp);
    return load_file_steps(e, idx, lr, frames, nframes, ir_rate, session_rate, shape, eq, damp, rq);
}

int mc_load_ir_filter(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate, uint32_t session_rate,
                      const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail, const mc_ir_phase* phase,
                      const mc_ir_filter* filter, const float* filter_lr, uint64_t filter_frames) {
    StepRequest rq;
    rq.tail = tail, rq.phase = phase, rq.filter = filter, rq.filter_lr = filter_lr, rq.filter_frames = filter_frames;
    if (!rq.normalise().any()) return mc_load_ir_damped(e, idx, lr, frames, nframes, ir_rate, session_rate, shape, eq, damp);
    return load_file_steps(e, idx, lr, frames, nframes, ir_rate, session_rate, shape, eq, damp, rq);
}

int mc_load_ir_sweep_phase(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, const mc_sweep* sweep, int64_t offset,
                           uint64_t ir_frames, const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail,
                           const mc_ir_phase* phase) {
    StepRequest rq;
    rq.tail = tail, rq.phase = phase;
    if (!rq.normalise().any()) return mc_load_ir_sweep(e, idx, lr, frames, nframes, sweep, offset, ir_frames, shape, eq, damp);
    return load_sweep_steps(e, idx, lr, frames, nframes, sweep, offset, ir_frames, shape, eq, damp, rq);
}

int mc_load_ir_sweep_filter(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, const mc_sweep* sweep, int64_t offset,
                            uint64_t ir_frames, const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail,
                            const mc_ir_phase* phase, const mc_ir_filter* filter, const float* filter_lr, uint64_t filter_frames) {
    StepRequest rq;
    rq.tail = tail, rq.phase = phase, rq.filter = filter, rq.filter_lr = filter_lr, rq.filter_frames = filter_frames;
    if (!rq.normalise().any()) return mc_load_ir_sweep(e, idx, lr, frames, nframes, sweep, offset, ir_frames, shape, eq, damp);
    return load_sweep_steps(e, idx, lr, frames, nframes, sweep, offset, ir_frames, shape, eq, damp, rq);
}

int mc_load_ir_match(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate, uint32_t session_rate,
                     const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail, const mc_ir_phase* phase,
                     const mc_ir_filter* filter, const float* filter_lr, uint64_t filter_frames, const mc_ir_match* match, const float* target_lr,
                     uint64_t target_frames) {
    StepRequest rq;
    rq.tail = tail, rq.phase = phase, rq.filter = filter, rq.filter_lr = filter_lr, rq.filter_frames = filter_frames,
        rq.match = match, rq.target_lr = target_lr, rq.target_frames = target_frames;
    if (!rq.normalise().any()) return mc_load_ir_damped(e, idx, lr, frames, nframes, ir_rate, session_rate, shape, eq, damp);
    return load_file_steps(e, idx, lr, frames, nframes, ir_rate, session_rate, shape, eq, damp, rq);
}

int mc_load_ir_sweep_match(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, const mc_sweep* sweep, int64_t offset,
                           uint64_t ir_frames, const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail,
                           const mc_ir_phase* phase, const mc_ir_filter* filter, const float* filter_lr, uint64_t filter_frames,
                           const mc_ir_match* match, const float* target_lr, uint64_t target_frames) {
    StepRequest rq;
    rq.tail = tail, rq.phase = phase, rq.filter = filter, rq.filter_lr = filter_lr, rq.filter_frames = filter_frames,
        rq.match = match, rq.target_lr = target_lr, rq.target_frames = target_frames;
    if (!rq.normalise().any()) return mc_load_ir_sweep(e, idx, lr, frames, nframes, sweep, offset, ir_frames, shape, eq, damp);
    return load_sweep_steps(e, idx, lr, frames, nframes, sweep, offset, ir_frames, shape, eq, damp, rq);
}

int mc_load_ir_parts(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate, uint32_t session_rate,
                     const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail, const mc_ir_phase* phase,
                     const mc_ir_filter* filter, const float* filter_lr, uint64_t filter_frames, const mc_ir_match* match, const float* target_lr,
                     uint64_t target_frames, const mc_ir_parts* parts) {
    StepRequest rq;
    rq.tail = tail, rq.phase = phase, rq.filter = filter, rq.filter_lr = filter_lr, rq.filter_frames = filter_frames,
        rq.match = match, rq.target_lr = target_lr, rq.target_frames = target_frames, rq.parts = parts;
    if (!rq.normalise().any()) return mc_load_ir_damped(e, idx, lr, frames, nframes, ir_rate, session_rate, shape, eq, damp);
    return load_file_steps(e, idx, lr, frames, nframes, ir_rate, session_rate, shape, eq, damp, rq);
}

int mc_load_ir_sweep_parts(mc_engine* e, uint64_t idx, const float* lr, uint64_t frames, uint64_t nframes, const mc_sweep* sweep, int64_t offset,
                           uint64_t ir_frames, const mc_ir_shape* shape, const mc_ir_eq* eq, const mc_ir_damp* damp, const mc_ir_tail* tail,
                           const mc_ir_phase* phase, const mc_ir_filter* filter, const float* filter_lr, uint64_t filter_frames,
                           const mc_ir_match* match, const float* target_lr, uint64_t target_frames, const mc_ir_parts* parts) {
    StepRequest rq;
    rq.tail = tail, rq.phase = phase, rq.filter = filter, rq.filter_lr = filter_lr, rq.filter_frames = filter_frames,
        rq.match = match, rq.target_lr = target_lr, rq.target_frames = target_frames, rq.parts = parts;
    if (!rq.normalise().any()) return mc_load_ir_sweep(e, idx, lr, frames, nframes, sweep, offset, ir_frames, shape, eq, damp);
    return load_sweep_steps(e, idx, lr, frames, nframes, sweep, offset, ir_frames, shape, eq, damp, rq);
}

void mc_default_ir_parts(mc_ir_parts* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->mode = MC_PARTS_OFF;
    for (int k = 0; k < PT_PARTS; k++) p->width[k] = 1.f;
}

int mc_ir_parts_plan(const mc_ir_parts* p, uint64_t frames, double out[4], double coef[12]) {
    if (!p) return fail(MC_ERR_ARG, "null parts");
    if (const char* bad = parts_check(p)) return fail(MC_ERR_ARG, "%s", bad);
    if (!frames) return fail(MC_ERR_ARG, "empty IR");
    if (const char* bad = parts_check_frames(p, frames)) return fail(MC_ERR_ARG, "%s", bad);
    if (!out || !coef) return fail(MC_ERR_ARG, "null out");
    const PartsStep s = parts_step(*p, frames);
    out[0] = (double)s.Fo, out[1] = (double)s.s[0], out[2] = (double)s.s[1], out[3] = (double)parts_device_bytes(s);
    for (int k = 0; k < PT_PARTS; k++) std::copy(s.c[k], s.c[k] + 4, coef + 4 * k);
    return MC_OK;
}

int mc_ir_parts_at(mc_ir_parts* parts, uint64_t onset, uint64_t direct_frames, uint64_t early_frames) {
    if (!parts) return fail(MC_ERR_ARG, "null parts");
    if (parts->struct_size != sizeof(mc_ir_parts)) return fail(MC_ERR_ARG, "mc_ir_parts struct_size mismatch");
    if (early_frames < direct_frames) return fail(MC_ERR_ARG, "early_frames %llu below direct_frames %llu", (unsigned long long)early_frames, (unsigned long long)direct_frames);
    if (onset > PT_MAX_BOUNDARY || early_frames > PT_MAX_BOUNDARY || onset + early_frames > PT_MAX_BOUNDARY)
        return fail(MC_ERR_ARG, "the boundary at onset %llu + %llu frames lies above 2^40", (unsigned long long)onset, (unsigned long long)early_frames);
    parts->direct_end = onset + direct_frames;
    parts->early_end = onset + early_frames;
    return MC_OK;
}

int mc_ir_parts_info(const mc_engine* e, uint64_t idx, double out[10]) { return ir_fact(e, idx, FACT_PARTS, 10, "was not loaded with a parts step", out); }

void mc_default_ir_match(mc_ir_match* m) {
    if (!m) return;
    std::memset(m, 0, sizeof(*m));
    m->struct_size = (uint32_t)sizeof(*m);
    m->mode = MC_MATCH_OFF;
    m->phase = MC_MATCH_MINIMUM;
    m->link = 1;
    m->per_octave = 12;
    m->lo_hz = 20.0;
    m->octaves = 1.0 / 3.0;
    m->amount = 1.f;
    m->boost_db = 12.f;
    m->cut_db = 24.f;
    m->floor_db = 120.f;
}

int mc_ir_match_plan(const mc_ir_match* m, uint64_t frames, uint64_t target_frames, uint32_t session_rate, double out[6]) {
    if (!m) return fail(MC_ERR_ARG, "null match");
    if (const char* bad = match_check(m)) return fail(MC_ERR_ARG, "%s", bad);
    if (!frames) return fail(MC_ERR_ARG, "empty IR");
    mc_ir_match at = *m;  // (both lengths are at the session's rate already; off is planned as a target)
    at.rate = 0;
    if (at.mode == MC_MATCH_OFF) at.mode = MC_MATCH_TARGET;
    uint64_t G = 0;
    if (const char* bad = match_check_load(&at, session_rate, frames, target_frames, &G)) return fail(MC_ERR_ARG, "%s", bad);
    if (!out) return fail(MC_ERR_ARG, "null out");
    const MatchStep s = match_step(at, session_rate, frames, G);
    out[0] = (double)s.Nfft, out[1] = (double)s.fft.passes, out[2] = (double)match_device_bytes(s), out[3] = (double)s.Fo, out[4] = (double)s.J;
    out[5] = (double)s.window_bins;
    return MC_OK;
}

int mc_ir_match_info(const mc_engine* e, uint64_t idx, double out[12]) { return ir_fact(e, idx, FACT_MATCH, 12, "was not loaded with a match step", out); }

int mc_ir_match_curve(const mc_engine* e, uint64_t idx, double* hz, double* before_db, double* gain_db, uint32_t cap) {
    double info[12];
    if (const int rc = ir_fact(e, idx, FACT_MATCH, 12, "was not loaded with a match step", info)) return rc;
    const std::vector<double>& c = e->irs[idx].match_curve;
    const size_t J = c.size() / 5;
    if (!hz || !before_db || !gain_db) return fail(MC_ERR_ARG, "null argument");
    if (cap < J) return fail(MC_ERR_ARG, "cap %u below the curve's %llu points", cap, (unsigned long long)J);
    std::copy(c.begin(), c.begin() + J, hz);
    std::copy(c.begin() + J, c.begin() + 3 * J, before_db);
    std::copy(c.begin() + 3 * J, c.end(), gain_db);
    return (int)J;
}

void mc_default_ir_filter(mc_ir_filter* f) {
    if (!f) return;
    std::memset(f, 0, sizeof(*f));
    f->struct_size = (uint32_t)sizeof(*f);
    f->op = MC_FILTER_OFF;
    f->channels = MC_FILTER_STEREO;
    f->reg_db = 60.f;
}

int mc_ir_filter_plan(const mc_ir_filter* f, uint64_t frames, uint64_t filter_frames, double out[4]) {
    if (!f) return fail(MC_ERR_ARG, "null filter");
    if (const char* bad = filter_check(f)) return fail(MC_ERR_ARG, "%s", bad);
    if (!frames) return fail(MC_ERR_ARG, "empty IR");
    if (const char* bad = filter_check_frames(f, frames, filter_frames)) return fail(MC_ERR_ARG, "%s", bad);
    if (!out) return fail(MC_ERR_ARG, "null out");
    const FilterStep s = filter_step(*f, frames, filter_frames);
    out[0] = (double)s.Nfft, out[1] = (double)s.fft.passes, out[2] = (double)filter_device_bytes(s), out[3] = (double)s.Fo;
    return MC_OK;
}

int mc_ir_filter_info(const mc_engine* e, uint64_t idx, double out[10]) { return ir_fact(e, idx, FACT_FILTER, 10, "was not loaded with a filter step", out); }

int mc_ir_phase_info(const mc_engine* e, uint64_t idx, double out[8]) { return ir_fact(e, idx, FACT_PHASE, 8, "was not loaded with a phase step", out); }

int mc_ir_shape_info(const mc_engine* e, uint64_t idx, double out[8]) { return ir_fact(e, idx, FACT_SHAPE, 8, "was not loaded with a shape", out); }

int mc_num_irs(const mc_engine* e) { return e ? e->nirs : 0; }

int mc_ir_info(const mc_engine* e, uint64_t idx, double out[6]) {
    if (!e || !out || idx >= (uint64_t)kMaxIrs || !(e->irs[idx].d_H || e->irs[idx].d_S)) return fail(MC_ERR_ARG, "IR %llu not loaded", (unsigned long long)idx);
    for (int i = 0; i < 4; i++) out[i] = e->irs[idx].sums[i];
    out[4] = (double)e->irs[idx].taps;
    out[5] = (double)e->irs[idx].P;
    return MC_OK;
}

int mc_set_params(mc_engine* e, int half, const mc_cc_value* v) {
    if (!e || !v || half < 0 || half > 1) return fail(MC_ERR_ARG, "bad argument");
    e->ph.update([&](mc_cc_value (&cc)[2]) { cc[half] = *v; });
    return MC_OK;
}

int mc_get_params(const mc_engine* e, int half, mc_cc_value* v) {
    if (!e || !v || half < 0 || half > 1) return fail(MC_ERR_ARG, "bad argument");
    mc_cc_value cc[2];
    e->ph.sample(cc);
    *v = cc[half];
    return MC_OK;
}

int mc_handle_cc(mc_engine* e, int half, const uint8_t ccmap[8], uint8_t m2, int val) {
    // handleCC, conv.cu:255-276
    if (!e || !ccmap || half < 0 || half > 1) return fail(MC_ERR_ARG, "bad argument");
    const uint64_t nb = (uint64_t)e->nirs;
    e->ph.update([&](mc_cc_value (&cc)[2]) {
        mc_cc_value& v = cc[half];
        if (ccmap[0] == m2) {
            v.select = (uint64_t)val * nb / 0x80;
            v.vsteps = v.speed;
        }
        if (ccmap[1] == m2) v.predelay = (uint64_t)val * MC_MAX_PREDELAY / 0x80;
        if (ccmap[2] == m2) v.dry = val / 128.0f;
        if (ccmap[3] == m2) v.wet = val / 128.0f;
        if (ccmap[5] == m2) v.panDry = val / 64.0f - 1;
        if (ccmap[6] == m2) v.panWet = val / 64.0f - 1;
        if (ccmap[7] == m2) v.level = val / 128.0f;
        if (ccmap[4] == m2) {
            v.speed = ((uint64_t)val * MC_MAX_SPEED) / 0x80;
            if (v.vsteps > v.speed) v.vsteps = v.speed;
        }
    });
    return MC_OK;
}

int mc_process(mc_engine* e, const float* in1, const float* in2, float* outL, float* outR, uint64_t nframes) {
    if (!e) return fail(MC_ERR_ARG, "null engine");
    if (nframes != (uint64_t)MC_BLOCK * e->pm)
        return fail(MC_ERR_ARG, "nframes must be %d (got %llu)", MC_BLOCK * e->pm, (unsigned long long)nframes);
    HIP_TRY(hipSetDevice(e->device));
    // the reference brackets its GPU work with events (conv.cu:299-302, 454-462); the call below
    // returns only when the output is on the host, so a host clock around it measures a superset
    const auto t0 = std::chrono::steady_clock::now();
    // 256-frame periods take the fused single-block path; 512 / 1024 run as one small zero-copy batch
    // (partition shards keep the batch kernels: their low partitions are not the IR's first ones)
    const bool whole_ir = e->cfg.part_begin == 0 && e->cfg.part_end == 0;
    int rc = e->sf ? sf_process(e, in1, in2, outL, outR) : e->pm == 1 ? process_one(e, in1, in2, outL, outR)
                        : (whole_ir ? process_period_fused(e, in1, in2, outL, outR) : process_period(e, in1, in2, outL, outR));
    if (rc) return rc;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (++e->nruns > 0) e->runtime_ms += ms;  // first 10 calls discarded, conv.h:80
    return MC_OK;
}

void* mc_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        fail(MC_ERR_NOMEM, "mc_host_alloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}

void mc_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int mc_process_batch(mc_engine* e, const float* in1, const float* in2, float* outL, float* outR, uint64_t nblocks) {
    if (!e) return fail(MC_ERR_ARG, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    if (e->sf) return sf_batch_host(e, in1, in2, outL, outR, (int)std::min<uint64_t>(nblocks, 1u << 30));
    return process_host(e, in1, in2, outL, outR, (int)std::min<uint64_t>(nblocks, 1u << 30));
}

int mc_process_batch_device(mc_engine* e, const float* d_in1, const float* d_in2, float* d_outL, float* d_outR, uint64_t nblocks) {
    if (!e || !d_in1 || !d_in2 || !d_outL || !d_outR) return fail(MC_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    const int T = (int)std::min<uint64_t>(nblocks, 1u << 30);
    if (e->sf) return sf_batch_device(e, d_in1, d_in2, d_outL, d_outR, T);
    int rc = run_front(e, d_in1, d_in2, T, nullptr, 0, T, d_outL, d_outR);
    if (rc) return rc;
    return run_back(e, d_in1, d_in2, nullptr, d_outL, d_outR, T);
}

int mc_process_batch_slice_device(mc_engine* e, const float* d_in1, const float* d_in2, float* d_outL, float* d_outR,
                                  uint64_t nblocks, uint64_t first, uint64_t count) {
    if (!e || !d_in1 || !d_in2 || !d_outL || !d_outR) return fail(MC_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    const int T = (int)std::min<uint64_t>(nblocks, 1u << 30);
    if (e->sf) return fail(MC_ERR_ARG, "the single-transform form has no block slices");
    if (first > (uint64_t)T || count > (uint64_t)T) return fail(MC_ERR_ARG, "slice outside the batch");
    int rc = run_front(e, d_in1, d_in2, T, nullptr, (int)first, (int)count, d_outL, d_outR);
    if (rc) return rc;
    return run_back(e, d_in1, d_in2, nullptr, d_outL, d_outR, T);
}

int mc_partial_batch_device(mc_engine* e, const float* d_in1, const float* d_in2, float* d_partial, uint64_t nblocks) {
    if (!e || !d_in1 || !d_in2 || !d_partial) return fail(MC_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    const int T = (int)std::min<uint64_t>(nblocks, 1u << 30);
    if (e->sf) return fail(MC_ERR_ARG, "the single-transform form has no partition shards");
    return run_front(e, d_in1, d_in2, T, d_partial, 0, T);
}

int mc_finish_batch_device(mc_engine* e, const float* d_in1, const float* d_in2, const float* d_wet_sum, float* d_outL,
                           float* d_outR, uint64_t nblocks) {
    if (!e) return fail(MC_ERR_ARG, "null engine");
    if (e->sf) return fail(MC_ERR_ARG, "the single-transform form has no partition shards");
    const bool want_out = d_outL || d_outR || d_wet_sum;
    if (want_out && (!d_in1 || !d_in2 || !d_wet_sum || !d_outL || !d_outR)) return fail(MC_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    const int T = (int)std::min<uint64_t>(nblocks, 1u << 30);
    if (T <= 0 || T > e->Tmax) return fail(MC_ERR_ARG, "nblocks outside range");
    return run_back(e, d_in1, d_in2, d_wet_sum, want_out ? d_outL : nullptr, d_outR, T);
}

int mc_finish_batch_slice_device(mc_engine* e, const float* d_in1, const float* d_in2, const float* d_wet_sum_slice, float* d_outL,
                                 float* d_outR, uint64_t nblocks, uint64_t first, uint64_t count) {
    if (!e || !d_in1 || !d_in2 || !d_wet_sum_slice || !d_outL || !d_outR) return fail(MC_ERR_ARG, "null argument");
    if (e->sf) return fail(MC_ERR_ARG, "the single-transform form has no partition shards");
    HIP_TRY(hipSetDevice(e->device));
    const int T = (int)std::min<uint64_t>(nblocks, 1u << 30);
    if (T <= 0 || T > e->Tmax) return fail(MC_ERR_ARG, "nblocks outside range");
    if (first >= (uint64_t)T || count == 0 || count > (uint64_t)T - first) return fail(MC_ERR_ARG, "slice outside the batch");
    return run_back(e, d_in1, d_in2, d_wet_sum_slice, d_outL, d_outR, T, false, (int)first, (int)count);
}

int mc_sync(mc_engine* e) {
    if (!e) return fail(MC_ERR_ARG, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    int rc = drain_post(e);
    if (!rc) unpark(e);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return MC_OK;
}

int mc_fence(mc_engine* e) {
    if (!e) return fail(MC_ERR_ARG, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    return fence_post(e);
}

int mc_fence_older(mc_engine* e) {
    if (!e) return fail(MC_ERR_ARG, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    if (!e->pipelined || e->batch_seq == 0) return MC_OK;
    const int older = (int)(e->batch_seq & 1);  // the most recent batch had parity (batch_seq - 1) & 1
    if (e->post_pending[older]) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_post[older], 0));
    return MC_OK;
}

int mc_set_stream(mc_engine* e, void* s) {
    if (!e) return fail(MC_ERR_ARG, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    {
        int rc = drain_post(e);
        if (!rc) unpark(e);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->stream = s ? (hipStream_t)s : (hipStream_t)e->own_stream;
    return MC_OK;
}

void* mc_get_stream(mc_engine* e) { return e ? (void*)e->stream : nullptr; }

double mc_avg_runtime_ms(const mc_engine* e) { return (e && e->nruns > 0) ? e->runtime_ms / e->nruns : 0.0; }  // conv.h:61

int mc_enable_kernel_timing(mc_engine* e, int on) {
    if (!e) return fail(MC_ERR_ARG, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    if (on && !e->kt) {
        HIP_TRY(make_group(e->kt, (size_t)2 * MC_STAMP_WGS * kStampSlots));
        for (int i = 0; i < kEvPool; i++) e->kev_stamped[i] = false;
    }
    if (!on) {
        int rc = drain_kernel_events(e);
        if (rc) return rc;
    }
    e->ktiming = on != 0;
    return MC_OK;
}

int mc_get_kernel_stats(mc_engine* e, mc_kernel_stats* out, int reset) {
    if (!e || !out) return fail(MC_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    int rc = drain_kernel_events(e);
    if (rc) return rc;
    *out = e->ks;
    if (reset) {
        uint32_t res = e->ks.resident, parts = e->ks.partitions, lv = e->ks.fast_levels;
        std::memset(&e->ks, 0, sizeof(e->ks));
        e->ks.resident = res;
        e->ks.partitions = parts;
        e->ks.fast_levels = lv;
    }
    return MC_OK;
}

uint64_t mc_algorithmic_bytes_per_block(const mc_engine* e) {
    // 4 IR paths + 2 delay-line inputs, P partitions, 256 bins x 8 B
    if (!e) return 0;
    if (e->sf) return 24ull * e->cfg.n_ref;  // four half spectra (4 N/2 x 8 B) + the input window (2 N x 4 B), per call
    mc_cc_value cc[2];
    e->ph.sample(cc);
    const IrEntry& a = e->irs[cc[0].select % kMaxIrs];
    const IrEntry& b = e->irs[cc[1].select % kMaxIrs];
    int P = std::max(a.P, b.P);
    if (e->cfg.part_end) P = std::max(0, std::min<int>(P, (int)e->cfg.part_end) - (int)e->cfg.part_begin);
    return (uint64_t)(4 + 2) * (uint64_t)P * MC_NB * (e->half ? 4ull : 8ull);
}

uint64_t mc_blocks_processed(const mc_engine* e) { return e ? e->t_abs : 0; }

uint64_t mc_preferred_batch(const mc_engine* e, uint64_t at_most) {
    if (!e) return 0;
    at_most = std::min<uint64_t>(at_most, (uint64_t)e->Tmax);
    if (e->sf) return at_most - at_most % (uint64_t)e->pm;
    int pmax = 0;
    for (int i = 0; i < kMaxIrs; i++)
        if (e->irs[i].d_H) pmax = std::max(pmax, round_up(e->irs[i].P, 16));
    const bool shard = e->cfg.part_begin || e->cfg.part_end;
    if (shard) {  // taps of the shard's own run of partitions
        int pb, pe;
        partition_range(e, pmax, &pb, &pe);
        pmax = pe - pb;
    }
    uint64_t chunk = 0;
    // overlap-save segments of 16384 - P16 blocks (ossave.hip.h): whole segments waste nothing
    if (e->os_on && !e->half && !e->pipelined && !shard && pmax > 0 && (int64_t)pmax * MC_B <= OS_N / 2) {
        const uint64_t hopb = (uint64_t)(OS_N / MC_B - pmax);
        if (at_most >= hopb && at_most >= (uint64_t)e->os_min_blocks) return at_most / hopb * hopb;
    }
    if (e->fft2 && !e->half && pmax >= 16) {
        if (e->fft2_fused && pmax <= kG2Pmax) chunk = (uint64_t)(G2_N - pmax + 1);
        else if (pmax <= F2_N / 2) chunk = (uint64_t)(F2_N - pmax + 1);
    }
    if (!chunk || at_most < chunk) return at_most >= 8 ? (at_most & ~(uint64_t)7) : at_most;
    return ((at_most + 1) / chunk * chunk - 1) & ~(uint64_t)7;
}

int mc_debug_read(mc_engine* e, int which, uint64_t idx, void* dst, uint64_t off, uint64_t bytes, uint64_t dims[4]) {
    if (!e) return fail(MC_ERR_ARG, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    if (e->sf && which == 17) return fail(MC_ERR_STATE, "the single-transform form keeps no taps");
    if (e->sf) {  // single-transform form: 0 = an IR's spectra [H_L | H_R] (float2, n_ref / 2 bins each, bin d + (n_ref / 512) c at [d][c]), 4 = the accumulators [2][512][n_ref / 512]
        if (dims) dims[0] = dims[1] = dims[3] = e->cfg.n_ref, dims[2] = (uint64_t)e->Tmax;
        if (!dst || !bytes) return MC_OK;
        const char* src = nullptr;
        uint64_t cap = 0;
        if (which == 0 && idx < (uint64_t)kMaxIrs && e->irs[idx].d_S) src = (const char*)e->irs[idx].d_S.get(), cap = sizeof(float2) * e->cfg.n_ref;
        else if (which == 4) src = (const char*)e->sf->d_acc.get(), cap = sizeof(float) * 2 * e->cfg.n_ref;
        else return fail(MC_ERR_ARG, "nothing to read for item %d in the single-transform form", which);
        if (off > cap || bytes > cap - off) return fail(MC_ERR_ARG, "read outside the buffer");
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipMemcpy(dst, src + off, bytes, hipMemcpyDeviceToHost));
        return MC_OK;
    }
    if (dims) {
        dims[0] = (uint64_t)e->Pstride;
        dims[1] = (uint64_t)e->ring;
        dims[2] = (uint64_t)e->Tmax;
        dims[3] = (uint64_t)e->wr;
    }
    if (!dst || !bytes) return MC_OK;
    if (which == 7 || which == 8) {  // generation of the parameter pair the last process call sampled (7) / published last (8): no stream access
        mc_cc_value cc[2];
        const uint64_t g = which == 7 ? e->last_gen : e->ph.sample(cc);
        if (off + bytes > sizeof(uint64_t)) return fail(MC_ERR_ARG, "read beyond the generation word");
        std::memcpy(dst, reinterpret_cast<const char*>(&g) + off, bytes);
        return MC_OK;
    }
    if (which == 10) {  // batches by the form their partition sums took {fused, split second-level transform, resident MAC}: no stream access
        if (off + bytes > sizeof(e->n_mac_form)) return fail(MC_ERR_ARG, "read beyond the counters");
        std::memcpy(dst, reinterpret_cast<const char*>(e->n_mac_form) + off, bytes);
        return MC_OK;
    }
    if (which == 11) {  // overlap-save form: {batches that took it, spectra builds}: no stream access
        if (off + bytes > sizeof(e->n_os)) return fail(MC_ERR_ARG, "read beyond the counters");
        std::memcpy(dst, reinterpret_cast<const char*>(e->n_os) + off, bytes);
        return MC_OK;
    }
    if (which == 9) {  // Q8 regime, batches: {cut terms summed by k_drop_fft for the whole batch, by the forward transforms (k_fwd<true>), in the time domain}: no stream access
        const uint64_t c[4] = {e->n_drop_fft, e->n_drop_ahead, e->n_drop_tiles, e->n_drop_carried};
        if (off + bytes > sizeof(c)) return fail(MC_ERR_ARG, "read beyond the counters");
        std::memcpy(dst, reinterpret_cast<const char*>(c) + off, bytes);
        return MC_OK;
    }
    if (which == 16) {  // 256-frame tails by the form their partition 0 took {frequency domain, time domain}: counted on the device, read behind the stream
        unsigned c[2] = {0, 0};
        if (off + bytes > sizeof(c)) return fail(MC_ERR_ARG, "read beyond the counters");
        if (e->d_tailform) {
            unpark(e);
            HIP_TRY(hipStreamSynchronize(e->stream));
            HIP_TRY(hipMemcpy(c, e->d_tailform, sizeof(c), hipMemcpyDeviceToHost));
        }
        std::memcpy(dst, reinterpret_cast<const char*>(c) + off, bytes);
        return MC_OK;
    }
    if (which == 6) {  // host-side counters of the JACK path's parked periods {used, gave up on their own, told to give up}: no stream access
        const uint64_t c[3] = {e->n_park_hit, e->n_park_timeout, e->n_park_cancel};
        if (off + bytes > sizeof(c)) return fail(MC_ERR_ARG, "read beyond the counters");
        std::memcpy(dst, reinterpret_cast<const char*>(c) + off, bytes);
        return MC_OK;
    }
    if ((which >= 18 && which <= 20) && !e->half) return fail(MC_ERR_STATE, "item %d: the engine keeps no fp16 copies (precision = fp32)", which);
    const char* src = nullptr;
    uint64_t cap = 0;
    switch (which) {
        case 0:  // (items 0, 18 and 20 also read the merged-IR entries kMaxIrs .. kMaxIrs + kMixIrs - 1)
            if (idx >= (uint64_t)(kMaxIrs + kMixIrs) || !e->irs[idx].d_H) return fail(MC_ERR_ARG, "IR not loaded");
            src = (const char*)e->irs[idx].d_H.get();
            cap = sizeof(float4) * (uint64_t)MC_NB * e->Pstride;
            break;
        case 18:  // the fp16 copy of IR idx's spectra, scaled by item 20 (uint2 [256][pstride])
            if (idx >= (uint64_t)(kMaxIrs + kMixIrs) || !e->irs[idx].d_H || !e->irs[idx].d_H16) return fail(MC_ERR_ARG, "IR not loaded");
            src = (const char*)e->irs[idx].d_H16.get();
            cap = sizeof(uint2) * (uint64_t)MC_NB * e->Pstride;
            break;
        case 19: src = (const char*)e->d_fdl16.get(); cap = sizeof(uint2) * (uint64_t)MC_NB * e->ring; break;
        case 20: {  // scale16 of IR idx (one float): a host-side word, read behind the stream like the copy it belongs to
            if (idx >= (uint64_t)(kMaxIrs + kMixIrs) || !e->irs[idx].d_H || !e->irs[idx].d_H16) return fail(MC_ERR_ARG, "IR not loaded");
            if (off + bytes > sizeof(float)) return fail(MC_ERR_ARG, "read beyond the scale");
            unpark(e);
            HIP_TRY(hipStreamSynchronize(e->stream));
            std::memcpy(dst, reinterpret_cast<const char*>(&e->irs[idx].scale16) + off, bytes);
            return MC_OK;
        }
        case 21: src = (const char*)e->d_slotgain.get(); cap = sizeof(float4) * (uint64_t)MC_MAXV * e->ring; break;
        case 17:  // the stored time-domain taps of IR idx (float2 [taps]: converted to the session's rate by mc_load_ir_resampled)
            if (idx >= (uint64_t)kMaxIrs || !e->irs[idx].d_h) return fail(MC_ERR_ARG, "IR not loaded");
            src = (const char*)e->irs[idx].d_h.get();
            cap = sizeof(float2) * e->irs[idx].taps;
            break;
        case 1: src = (const char*)e->d_fdl.get(); cap = sizeof(float4) * (uint64_t)MC_NB * e->ring; break;
        case 2: src = (const char*)e->d_Y; cap = sizeof(float4) * (uint64_t)MC_NB * y_capacity(e); break;
        case 3: src = (const char*)e->d_seg.get(); cap = sizeof(float) * (uint64_t)e->sr * 2 * FFT_N; break;
        case 4: src = (const char*)e->d_wet.get(); cap = sizeof(float) * 2 * (uint64_t)e->wr; break;
        case 5: src = (const char*)e->d_cring.get(); cap = sizeof(double) * 4 * (uint64_t)e->rc; break;
        case 12: src = (const char*)e->d_os_T.get(); cap = sizeof(float4) * e->d_os_T.size(); break;
        case 13: src = (const char*)e->d_os_SP.get(); cap = e->d_os_SP ? sizeof(float4) * (uint64_t)OS_ITEMS * OS_N2 * 2 : 0; break;
        case 14: src = (const char*)e->d_os_SP0.get(); cap = e->d_os_SP0 ? sizeof(float4) * 2 * (uint64_t)OS_N2 : 0; break;
        default: return fail(MC_ERR_ARG, "unknown buffer %d", which);
    }
    if (off + bytes > cap) return fail(MC_ERR_ARG, "read beyond buffer (%llu + %llu > %llu)", (unsigned long long)off, (unsigned long long)bytes, (unsigned long long)cap);
        unpark(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(dst, src + off, bytes, hipMemcpyDeviceToHost));
    return MC_OK;
}

}  // extern "C"
