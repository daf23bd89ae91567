/*
 * mcconv.h — C ABI of the MI355X partitioned-convolution reverb engine
 * (libmcconv.so, hand-written HIP for gfx950).
 *
 * This is the drop-in boundary for the reference's hot path: the entry points
 * are what a binding for limitz/cuda-audio's `Convolution` class needs, one
 * per reference interface (citations are file:line under the reference's src/):
 *
 *   mc_create            <- Convolution::Convolution(name, fftSize)   conv.h:52, conv.cu:142-195
 *   mc_destroy           <- (reference never frees; conv.h:53-54)
 *   mc_load_ir           <- Convolution::prepare(idx, wav, nframes)    conv.h:63, conv.cu:207-253
 *   mc_set_params /
 *   mc_get_params        <- public Convolution::cc[2].value            conv.h:33-50 (written by main.cu:49-70)
 *   mc_handle_cc         <- Convolution::onMidiMessage / handleCC      conv.h:65, conv.cu:255-285
 *   mc_process           <- Convolution::onProcess(nframes)            conv.h:59, conv.cu:287-466
 *   mc_avg_runtime_ms    <- Convolution::avgRuntime()                  conv.h:61, conv.cu:454-462
 *   mc_process_batch*    <- the same per-block path run over T consecutive
 *                           blocks in one call (throughput mode; new)
 *   mc_partial_* / mc_finish_* <- the two halves of a batch around the
 *                           cross-GPU sum when IR partitions are sharded (new)
 *
 * Plain pointers and sizes only; no C++ or torch types.  Every function
 * returns 0 on success or a negative mc_status, never throws, and leaves a
 * message for mc_last_error() (thread-local).  The caller keeps ownership of
 * every pointer it passes; the engine owns all device memory.
 *
 * Threading (mirrors SURVEY.md §8b): mc_process* is single-caller per engine;
 * mc_set_params / mc_handle_cc may be called from another thread (values are
 * sampled once at the start of each process call); mc_load_ir must not run
 * concurrently with mc_process*.
 */
#ifndef MCCONV_H
#define MCCONV_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MC_ABI_VERSION 1
#define MC_BLOCK 256          /* frames per internal block (and the default JACK period) */
#define MC_MAX_PREDELAY 8192  /* conv.h:26-28 */
#define MC_MAX_SPEED 1024     /* conv.h:22-24 */

typedef enum {
    MC_OK = 0,
    MC_ERR_ARG = -1,      /* bad argument / unsupported size */
    MC_ERR_HIP = -2,      /* HIP runtime error (message has the call) */
    MC_ERR_STATE = -3,    /* call not valid in this state (e.g. no IR loaded) */
    MC_ERR_NOMEM = -4
} mc_status;

typedef struct mc_engine mc_engine;

typedef struct {
    uint32_t struct_size;   /* sizeof(mc_config), for ABI evolution */
    int32_t device;         /* HIP device ordinal; -1 = current device */
    uint64_t n_ref;         /* the reference's fftSize (conv.h:52): IR truncation n_ref-1024
                               (conv.cu:239), Q1/Q2 window and 1/n_ref factors */
    uint32_t max_batch;     /* largest nblocks accepted by the device-buffer batch calls (1..1048576; the engine's rings and
                               scratch are sized by it: about 33 KB of device memory per block) */
    uint32_t max_partitions;/* 0 = derive from n_ref: ceil((n_ref-1024)/256) */
    uint32_t compat;        /* 1 = bug-compatible with conv.cu (DC/Nyquist terms Q1/Q2);
                               0 = plain linear convolution */
    uint32_t part_begin;    /* IR-partition shard [part_begin, part_end) computed by this */
    uint32_t part_end;      /* engine; 0,0 = all partitions (single GPU) */
    uint32_t stream_threshold; /* batches shorter than this use the streaming MAC kernel
                               (0 = default) */
    uint32_t precision;     /* 0 = fp32 spectra; 1 = fp16 storage of IR spectra and delay line for the
                               partition sweep (fp32 products and sums; the streaming kernel: single periods and batches
                               below 12288 blocks).  Longer settled batches take the overlap-save form in either precision
                               (its spectra are built from the fp32 taps: fp32 accuracy there).
                               The delay line's fp16 mirror holds 16 x the block's spectrum: full-scale input
                               (|x| <= 1, |X| <= 256) reaches 4096, and input beyond 16 times full scale overflows
                               the mirror (65504) to infinity.  Each IR's copy carries its own power-of-two scale,
                               2^(13 - e) for a largest spectrum entry in [2^(e-1), 2^e), the exponent held to at most
                               122 so that the scale times 16 and its reciprocal stay normal floats (at that limit, an IR
                               whose largest spectrum entry is below 2^-109, the reciprocal times a gain below 1 is a
                               subnormal float: exact enough only while the device keeps fp32 subnormals, as this build does) */
    uint32_t period;        /* JACK period the host will call mc_process with: 0/256, 512 or 1024 frames.  The
                               reference's per-call semantics (cross-fade step, DC/Nyquist and tail-drop windows)
                               follow this size; internally a period is 1, 2 or 4 blocks of 256.  Batch calls
                               take multiples of period/256 blocks. */
    uint32_t pipeline;      /* 1 = pipelined batches: mc_process_batch_device / _slice_device return once the MAC of
                               the batch is queued; its inverse transforms and post stage run on a second stream
                               under the MAC of the next batch.  The outputs of a call are complete, in the order of
                               the engine's stream, only after mc_fence (or mc_sync); its inputs must stay valid
                               until then.  Other calls drain the pipeline first.  0 = every call is complete in
                               stream order (default). */
    uint32_t form;          /* 0 = uniform-partitioned engine (default).  1 = the path in the reference's own shape
                               (BASELINE config 2): one n_ref-point transform per call, its live IR spectra stepped bin
                               by bin (conv.cu:15-32) and an n_ref-long running accumulator clamped at +-1 every call
                               (conv.cu:89-100) - the same samples while nothing saturates, the reference's samples
                               beyond.  n_ref <= 1048576, whole IR on one engine, fp32; no slices / shards / pipeline.
                               The environment variable MCCONV_FORM=single|partitioned overrides the field. */
    uint32_t reserved;
} mc_config;

/* mirrors Convolution::CC::value (conv.h:38-49); same defaults via mc_default_params */
typedef struct {
    uint64_t select;    /* index of the loaded IR used by this half */
    uint64_t predelay;  /* samples, [0, 8192]; half 0's value is used for both channels (conv.cu:412,415) */
    uint64_t speed;     /* cross-fade length in blocks, [0, 1024] */
    uint64_t vsteps;    /* remaining cross-fade steps (set to speed by a select CC) */
    float dry, wet, panDry, panWet, level;
} mc_cc_value;

typedef struct {
    uint64_t launches;      /* MAC-kernel launches timed so far */
    uint64_t blocks;        /* blocks those launches processed */
    double total_ms;        /* sum of the durations of those launches: HIP events around the launch; for the sweep of a
                               single period (a few microseconds) the kernel's own time stamps, first workgroup start to
                               last workgroup end */
    double last_ms;
    uint32_t resident;      /* 1 = the last launch used the resident (batch) kernel */
    uint32_t partitions;    /* partitions swept per block by the last launch */
    uint32_t fast_levels;   /* how the last long batch summed its partitions: 0 = direct-form MAC, 1..3 = fast-FIR form
                               with that many nested levels ((3/4)^levels of the multiply-adds); second-level transform
                               along the block axis instead of the MAC: 254 = its fused 8192-point form (one launch,
                               k_g2_mac: long batches with one set of gains where the overlap-save form does not apply),
                               255 = its split 16384-point form (k_f2_fwd + k_f2_prod: per-slot gains, IRs over 5632
                               partitions); 253 = overlap-save segments of 512 x 8192 frames (k_os_cols, k_os_rows, k_os_out:
                               the default for whole or block-sliced batches of >= 12288 blocks with one set of gains
                               outside the Q8 regime; `partitions` then holds the blocks of history per segment) */
    uint32_t reserved;
} mc_kernel_stats;

uint32_t mc_abi_version(void);
const char *mc_last_error(void);
void mc_default_config(mc_config *cfg);
void mc_default_params(mc_cc_value *v);

int mc_create(const mc_config *cfg, mc_engine **out);
void mc_destroy(mc_engine *e);
int mc_reset(mc_engine *e); /* zero all signal state (delay line, tails, cross-fade) */
/* change the JACK period (256, 512 or 1024 frames; see mc_config.period); resets the signal state */
int mc_set_period(mc_engine *e, uint32_t nframes);

/* lr: interleaved L,R float frames as WavFile holds them (already scaled, wav.cu Q5);
 * nframes: the reference's third prepare() argument (1024). Host pointer. */
int mc_load_ir(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes);
/* mc_load_ir for an IR recorded at ir_rate Hz in a session at session_rate Hz (both in [8000, 384000], else MC_ERR_ARG
 * before anything is touched): the frames are converted on the device to ceil(frames * session_rate / ir_rate) taps
 * (windowed sinc, Z = 64 zero crossings, Kaiser beta = 9, passband 0.955 of the lower Nyquist frequency, scaled by
 * ir_rate / session_rate so that sum h and the wet level stay put), then truncated and transformed exactly as
 * mc_load_ir's frames are.  Equal rates are mc_load_ir.  Host pointer, same rules as mc_load_ir.  No reference equivalent. */
int mc_load_ir_resampled(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate,
                         uint32_t session_rate);

/* Shaping of an IR on load: what a convolution reverb does to an impulse response before it convolves.  No reference
 * equivalent.  The engine-group interface (mcconv_group.h) has no counterpart: shaped loads are single-engine.
 *
 * Order of operations (lengths and positions are frames at the session's rate):
 *   1. the whole IR is converted to the session's rate when the rates differ (as by the resampled load); F frames;
 *   1a. (mc_load_ir_tail and mc_load_ir_sweep_tail only) every band of the F frames is cut at its knee or cross-faded there into
 *      decaying noise (mc_ir_tail below); F' frames leave the step and take the place of the F in everything that follows;
 *   1b. (mc_load_ir_phase and mc_load_ir_sweep_phase only) the F frames are replaced by the minimum-phase IR of the same
 *      magnitude response (mc_ir_phase below); F frames leave the step, and the onset search of step 2 sees them;
 *   1c. (mc_load_ir_filter and mc_load_ir_sweep_filter only) the F frames are convolved with a second impulse response, or that
 *      one is divided out of them (mc_ir_filter below); Fo frames leave the step and take the place of the F in everything
 *      that follows;
 *   1d. (mc_load_ir_match and mc_load_ir_sweep_match only) the F frames are given the smoothed spectrum of a target impulse
 *      response, or a flat or tilted one, by a match EQ (mc_ir_match below); Fo frames leave the step likewise;
 *   1e. (mc_load_ir_parts and mc_load_ir_sweep_parts only) the F frames are split into the direct sound, the early reflections
 *      and the late tail, each with a gain, a delay, a width and a balance of its own (mc_ir_parts below); Fo frames leave the
 *      step likewise, and the onset search of step 2 sees them;
 *   2. s0 = min(start, F); with trim_db < 0 the onset is the first frame m after s0 whose max(|L|, |R|) reaches
 *      peak * 10^(trim_db / 20) (float arithmetic; peak over all frames after s0); first = s0 + max(0, onset - pre_roll);
 *   3. n = min(F - first, length or unlimited, n_ref - nframes) frames are stored (n = 0: MC_ERR_ARG, nothing changes);
 *      every later step acts on those n, so a fade ends at the last stored tap and a normalisation measures what sounds;
 *   4. the n frames are reversed (MC_SHAPE_REVERSE);
 *   5. tap m is multiplied by 10^(-3 m / decay_t60);
 *   6. the last f = min(fade_out, n) taps by (1 + cos(pi (k + 1) / (f + 1))) / 2, k = 0 .. f - 1;
 *   6a. (mc_load_ir_damped only) the n taps are damped: a further decay per frequency band (mc_ir_damp below);
 *   6b. (mc_load_ir_eq and mc_load_ir_damped) the n taps run through the EQ bands, from rest at tap 0;
 *   7. everything by gain = target / peak or target / energy of the result (1 when that measure is 0);
 *   8. the taps are rounded to float and transformed as the plain load's are (steps 4-7 are carried in double). */
#define MC_SHAPE_REVERSE 1u
enum { MC_NORM_NONE = 0, MC_NORM_PEAK = 1, MC_NORM_ENERGY = 2 };
typedef struct {
    uint32_t struct_size;  /* sizeof(mc_ir_shape) */
    uint32_t flags;        /* MC_SHAPE_REVERSE; unknown bits: MC_ERR_ARG */
    uint64_t start;        /* frames skipped unconditionally at the front */
    uint64_t length;       /* frames kept from the first kept frame; 0 = all */
    uint64_t decay_t60;    /* 0 = off; else a further 60 dB of exponential decay at tap decay_t60 */
    uint64_t fade_out;     /* raised-cosine fade over the last fade_out stored taps (clamped to the stored length) */
    float trim_db;         /* [-120, 0]; 0 = no onset search; < 0: the threshold below the peak that marks the onset */
    uint32_t pre_roll;     /* frames kept before the onset */
    uint32_t normalize;    /* MC_NORM_* */
    float target;          /* PEAK: max |tap| = target; ENERGY: sqrt(sum (hL^2 + hR^2) / 2) = target; finite, > 0 */
} mc_ir_shape;

/* everything off */
void mc_default_ir_shape(mc_ir_shape *s);
/* The plain load (ir_rate = session_rate = 0) or the resampled load (both rates in [8000, 384000]) with `shape` applied
 * on the device between the conversion and the truncation.  The shape's fields and the rates are checked first, the
 * pointers after them, all before the engine or the device is touched: a refused load (MC_ERR_ARG, the message names
 * the field) leaves the engine as it was.  A shape with everything off is the plain or the resampled load itself, bit
 * for bit, and leaves no shape information.  The tap count, the sums and the taps the engine reports for the IR are
 * those of the shaped taps.  Two loads of the same frames with the same shape store the same bits. */
int mc_load_ir_shaped(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate,
                      uint32_t session_rate, const mc_ir_shape *shape);
/* out = {frames at the session's rate before shaping, onset frame (counted from `start`), first kept frame, stored taps,
 * gain applied, peak before the gain, energy before the gain, EQ bands applied (mc_load_ir_eq; else 0)}; MC_ERR_STATE for an IR whose last load was not shaped */
int mc_ir_shape_info(const mc_engine *e, uint64_t idx, double out[8]);

/* Equalisation of an IR on load: the EQ a convolution reverb has on its wet signal, applied to the impulse response once
 * (the wet path is linear), so that the period and batch paths pay nothing.  No reference equivalent; single-engine, as
 * shaping is.
 *
 * Up to MC_EQ_MAX_BANDS bands in index order; MC_EQ_OFF bands are skipped and their other fields ignored.  Each band is
 * one biquad H(z) = (b0 + b1 z^-1 + b2 z^-2) / (a0 + a1 z^-1 + a2 z^-2) with the Audio-EQ-Cookbook (R. Bristow-Johnson)
 * coefficients, computed in double from the float fields: w0 = 2 pi freq_hz / session_rate, c = cos w0,
 * al = sin w0 / (2 q), A = 10^(gain_db / 40), r = 2 sqrt(A) al:
 *   LOWCUT    (2nd-order high-pass)  b = {(1 + c) / 2, -(1 + c), (1 + c) / 2}          a = {1 + al, -2 c, 1 - al}
 *   HIGHCUT   (2nd-order low-pass)   b = {(1 - c) / 2,   1 - c,  (1 - c) / 2}          a = {1 + al, -2 c, 1 - al}
 *   LOWSHELF   b = {A ((A + 1) - (A - 1) c + r),  2 A ((A - 1) - (A + 1) c), A ((A + 1) - (A - 1) c - r)}
 *              a = {   (A + 1) + (A - 1) c + r,    -2 ((A - 1) + (A + 1) c),    (A + 1) + (A - 1) c - r}
 *   HIGHSHELF  b = {A ((A + 1) + (A - 1) c + r), -2 A ((A - 1) + (A + 1) c), A ((A + 1) + (A - 1) c - r)}
 *              a = {   (A + 1) - (A - 1) c + r,     2 ((A - 1) - (A + 1) c),    (A + 1) - (A - 1) c - r}
 *   PEAK       b = {1 + al A, -2 c, 1 - al A}                                          a = {1 + al / A, -2 c, 1 - al / A}
 * all divided by a0.  The cuts ignore gain_db.
 *
 * EQ is step 6b of the order of operations above, after the fade (6) and before the normalisation (7): the peak, the
 * energy and the gain that are measured and reported are those of the equalised taps.  The filter starts at rest at stored
 * tap 0 and runs over the n stored taps in double through the whole cascade; its ringing past tap n - 1 is dropped (n
 * does not change); the rounding to float is step 8's. */
#define MC_EQ_MAX_BANDS 8
enum { MC_EQ_OFF = 0, MC_EQ_LOWCUT, MC_EQ_HIGHCUT, MC_EQ_LOWSHELF, MC_EQ_HIGHSHELF, MC_EQ_PEAK };
typedef struct {
    uint32_t kind;   /* MC_EQ_*; anything above MC_EQ_PEAK: MC_ERR_ARG */
    float freq_hz;   /* corner / centre frequency, [10, 0.45 session_rate] */
    float gain_db;   /* shelves and peak: [-36, 24]; the cuts do not look at it */
    float q;         /* [0.1, 32] */
} mc_eq_band;
typedef struct {
    uint32_t struct_size;  /* sizeof(mc_ir_eq) */
    uint32_t reserved;
    mc_eq_band band[MC_EQ_MAX_BANDS];
} mc_ir_eq;

/* every band MC_EQ_OFF, freq_hz = 1000, gain_db = 0, q = 0.70710678 */
void mc_default_ir_eq(mc_ir_eq *eq);
/* mc_load_ir_shaped (shape = NULL: everything off) with `eq` applied as step 6b.  Everything is checked before the engine or
 * the device is touched (MC_ERR_ARG, the message names the field, the engine stays as it was): struct_size, every kind, and
 * with a band on session_rate and ir_rate (both in [8000, 384000]; equal rates mean no conversion, 0 / 0 is refused because
 * the bands need the session's rate) and the on bands' freq_hz, q and gain_db; a non-null shape as by mc_load_ir_shaped.
 * With no band on the call is mc_load_ir_shaped itself (and so, with the shape off too, the plain or the resampled load),
 * bit for bit.  A load with a band on counts as shaped: mc_ir_shape_info reports it, out[7] holds the number of bands
 * applied, gain, peak and energy are those of the equalised taps.  The same frames, shape and bands store the same bits. */
int mc_load_ir_eq(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate,
                  uint32_t session_rate, const mc_ir_shape *shape, const mc_ir_eq *eq);
/* db[i] = 20 log10 |H(e^{j 2 pi hz[i] / rate})| of the cascade (0 with no band on).  Host arithmetic only: no engine, no HIP
 * call.  `eq` is checked as by mc_load_ir_eq with session_rate = rate. */
int mc_ir_eq_response(const mc_ir_eq *eq, uint32_t rate, const double *hz, uint32_t n, double *db);

/* Damping of an IR on load: a decay time per frequency band, the control a convolution reverb puts next to its decay time
 * (hi / lo damp).  mc_ir_shape.decay_t60 is one broadband envelope and an EQ band is time-invariant; damping splits the IR
 * into up to four bands and gives each an envelope of its own.  No reference equivalent; single-engine, as shaping is.
 *
 * Damping is step 6a of the order of operations above: after the fade (6), before the EQ bands (6b).  The normalisation (7),
 * mc_ir_shape_info's gain, peak and energy and mc_ir_info's sums are those of the damped taps (damped and equalised with
 * EQ on).  n does not change: what the filters ring past tap n - 1 is dropped, as for EQ.
 *
 * x = the n taps after step 6, as double; X = n_xovers (1 .. 3); rate = session_rate.
 *   Crossover filters.  For k = 1 .. X, P_k is x run from rest at tap 0 through two identical sections in cascade, each the
 *     HIGHCUT of the table above at xover_hz[k - 1] with q = (double)0.70710678f (coefficients in double from the float
 *     fields), in transposed direct form II, in double.  The bands are B_0 = P_1, B_j = P_(j+1) - P_j, B_X = x - P_X; they
 *     telescope to x.
 *   Envelopes.  o = min(origin, n), t(m) = max(m, o) - o, and for band j = 0 .. X, low to high,
 *     g_j[m] = decay_t60[j] ? exp2(-(t(m) 3 log2(10)) / decay_t60[j]) : 1, step 5's expression counted from o.
 *   Output.  y[m] = g_X[m] x[m] + sum over k = 1 .. X of (g_(k-1)[m] - g_k[m]) P_k[m], added in that order: sum_j g_j B_j
 *     rearranged so that X filters and no band buffer are needed.  Hence
 *       - equal decays give y = g x exactly (the filters drop out): the broadband envelope counted from o;
 *       - all decays 0, or origin >= n, give y = x.
 * Two sections per crossover, not one: with a single 12 dB / octave section an undamped low band leaks into the band above it
 * and dominates that band's late decay.  The complement x - P_X keeps a 6 dB / octave skirt whatever the order, so a band's
 * decay curve is bent, not straight: aiming by 1 / T = 1 / T_before + rate / decay_t60 is approximate and meant
 * to be iterated against mc_ir_decay. */
#define MC_DAMP_MAX_XOVERS 3
typedef struct {
    uint32_t struct_size;                        /* sizeof(mc_ir_damp) = 64 */
    uint32_t n_xovers;                           /* 0 = off: every other field ignored */
    float xover_hz[MC_DAMP_MAX_XOVERS];          /* the first n_xovers: finite, [10, 0.45 session_rate], strictly ascending */
    uint32_t reserved;
    uint64_t decay_t60[MC_DAMP_MAX_XOVERS + 1];  /* band j = 0 .. n_xovers, low to high: a further 60 dB at tap origin + decay_t60[j]; 0 = none */
    uint64_t origin;                             /* stored tap the envelopes start at (clamped to n) */
} mc_ir_damp;
/* off; xover_hz = {250, 2000, 8000}; decays 0; origin 0 */
void mc_default_ir_damp(mc_ir_damp *d);
/* mc_load_ir_eq (shape, eq = NULL: everything off) with `damp` applied as step 6a.  With damp NULL or n_xovers = 0 the call is
 * mc_load_ir_eq itself, bit for bit (and so, with shape and eq off too, the plain or the resampled load).  With damping on
 * everything is checked before the engine or the device is touched (MC_ERR_ARG, the message names the field, the engine stays
 * as it was), in this order: struct_size; n_xovers <= MC_DAMP_MAX_XOVERS; session_rate and ir_rate (both in [8000, 384000];
 * equal rates mean no conversion, 0 / 0 is refused because the crossovers need the session's rate); each used xover_hz and
 * their order; then shape and eq as by mc_load_ir_eq.  A damped load counts as shaped: mc_ir_shape_info reports it with its
 * eight slots as they are, mc_ir_damp_info the rest.  The same frames, shape, bands and damping store the same bits. */
int mc_load_ir_damped(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate,
                      uint32_t session_rate, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp);
/* out = {crossovers, origin used (o), bands with a decay, 0}; MC_ERR_STATE unless the IR's last load damped */
int mc_ir_damp_info(const mc_engine *e, uint64_t idx, double out[4]);
/* The quasi-static response at stored tap `tap` (m above, with o taken as `origin`): db[i] = 20 log10 |g_X + sum over k of
 * (g_(k-1) - g_k) H_k(e^{j 2 pi hz[i] / rate})^2|, H_k one section of crossover k: what a slowly decaying tone of that frequency
 * is scaled by at that time.  0 dB with damping off.  Host arithmetic only: no engine, no HIP call.  `d` is checked as by
 * mc_load_ir_damped with ir_rate = session_rate = rate. */
int mc_ir_damp_response(const mc_ir_damp *d, uint32_t rate, uint64_t tap, const double *hz, uint32_t n, double *db);

/* The decay of a loaded IR, measured on the device from the taps the engine convolves with (after conversion, shaping and
 * EQ): the readout a convolution reverb shows for the IR it has loaded, and what mc_ir_shape.decay_t60 is aimed with.  No
 * reference equivalent; single-engine, as shaping is.  x = the n stored taps as double, N = end ? min(end, n) : n; only taps
 * [0, N) are searched and measured.
 *   1. origin o: with onset_db < 0 the first m whose max(|L|, |R|) reaches peak * 10^(onset_db / 20) (float arithmetic, the
 *      shaped load's onset search); with onset_db = 0, o = 0;
 *   2. row group 0 is broadband, y = x.  Row group b >= 1 is x[0 .. N) run from rest at tap 0 (not at o: the filter has settled
 *      by the onset) through two identical sections in cascade, each the Audio-EQ-Cookbook band-pass with 0 dB peak gain,
 *      b = {al, 0, -al}, a = {1 + al, -2 c, 1 - al}, all divided by a0, with w0 = 2 pi centre_hz[b - 1] / rate, c = cos w0,
 *      al = sin w0 / (2 q), in double from the float fields (transposed direct form II);
 *   3. channel sets s = 0, 1, 2: e[m] = yL^2, yR^2, yL^2 + yR^2 for m in [o, N);
 *   4. EDC[m] = sum of e[k] over k in [m, N) (the Schroeder integral), E = EDC[o], L[m] = 10 log10(EDC[m] / E); with E = 0 the
 *      row's energy is 0 and every other entry is NaN;
 *   5. a decay time over (hi, lo) dB: S = {m : lo <= L[m] <= hi}; NaN when L[N - 1] > lo (the curve never gets there) or S has
 *      fewer than 2 taps; else a = the least-squares slope of L over x = m - min S and T = -60 / (a rate) seconds.  EDT uses
 *      (0, -10), T20 (-5, -25), T30 (-5, -35);
 *   6. k50 = o + floor(0.05 rate + 0.5), k80 = o + floor(0.08 rate + 0.5); C50 = 10 log10((E - EDC[k50]) / EDC[k50]) dB, NaN
 *      when k50 >= N or EDC[k50] = 0; C80 likewise; D50 = (E - EDC[k50]) / E with C50's NaN rule;
 *      Ts = sum (m - o) e[m] / E / rate seconds;
 *   7. rows[(b 3 + s) 8 ..] = {E, EDT, T20, T30, C50, C80, D50, Ts};
 *      curve[(b 3 + s) K + j] = max(L[o + floor(j (N - 1 - o) / (K - 1))], -400), K = curve_points.
 * The curve of a finite IR always bends down towards tap N - 1, because the integral runs out there: a time fitted over a
 * range that reaches into that bend reads short.  `end` is the caller's tool against a noise floor or a cut; no noise-floor
 * compensation is attempted here: mc_ir_floor (below) finds where the floor starts, which is what to pass as `end`, and
 * mc_load_ir_tail removes the floor from the IR itself. */
#define MC_DECAY_MAX_BANDS 10
#define MC_DECAY_MAX_CURVE 1024
typedef struct {
    uint32_t struct_size;     /* sizeof(mc_decay_query) */
    uint32_t rate;            /* the rate the stored taps are at, [8000, 384000] */
    uint32_t n_bands;         /* 0 .. MC_DECAY_MAX_BANDS band-passed rows after the broadband row */
    uint32_t curve_points;    /* 0, or 2 .. MC_DECAY_MAX_CURVE points of the decay curve per row */
    float centre_hz[MC_DECAY_MAX_BANDS]; /* [10, 0.45 rate] */
    float q;                  /* [0.1, 32]; per section; default 1.41421356 (one octave) */
    float onset_db;           /* [-120, 0]; 0 = time zero is tap 0; default -20 */
    uint64_t end;             /* taps [0, end) are analysed; 0 = all stored taps */
} mc_decay_query;
/* rate 44100, no bands, no curve, q sqrt 2, onset -20, end 0 */
void mc_default_decay_query(mc_decay_query *q);
/* rows: [(1 + n_bands) * 3 * 8]; curve: [(1 + n_bands) * 3 * curve_points], NULL when curve_points = 0; info = {origin tap,
 * taps analysed N}.  Checked in this order, all before the engine or the device is touched (MC_ERR_ARG, the message names the
 * field): the query (struct_size, rate, n_bands, curve_points - 1 is refused -, each used centre_hz, q, onset_db), the
 * pointers, idx (an unloaded index: "IR not loaded").  MC_ERR_STATE in the single-transform form, which keeps no taps.
 * Threading as mc_load_ir: not concurrently with mc_process*.  Runs on the engine's stream and returns when the results are in
 * the caller's arrays.  Nothing the engine holds changes: later outputs, the stored taps, mc_ir_info and mc_ir_shape_info are
 * bit for bit what they would have been.  Two calls with the same query on the same IR return the same bits. */
int mc_ir_decay(mc_engine *e, uint64_t idx, const mc_decay_query *q, double *rows, double *curve, uint64_t info[2]);

/* The noise floor of a loaded IR, measured on the device: where a captured IR (mc_load_ir_sweep) stops decaying and turns
 * into the hiss of the room and the recorder, by Lundeby's method, which ISO 3382 points to.  No reference equivalent;
 * single-engine.  The stored taps are only read; N, the origin o, the channel sets s = L, R, L + R and e[m], EDC[m] (with
 * EDC[N] = 0) are those of mc_ir_decay's steps 1, 3 and 4.
 *
 * Row groups.  Group 0 is broadband, y = x.  With X = n_xovers >= 1, group j + 1 is band B_j, j = 0 .. X, of mc_ir_damp's split
 *   of x[0 .. N): P_k = x through crossover k's two identical HIGHCUT sections (q = (double)0.70710678f) from rest at tap 0,
 *   B_0 = P_1, B_j = P_(j+1) - P_j, B_X = x - P_X: the bands mc_ir_tail acts on.
 * The search, per row, in double.  n1 = N - o, cap = floor(n1 / 16), tail = max(1, floor(tail_fraction n1)).
 *   means(w)  I = floor(n1 / w) intervals of w taps: P_i = (EDC[o + i w] - EDC[o + (i + 1) w]) / w, D_i = 10 log10 P_i,
 *             t_i = o + i w + (w - 1) / 2;
 *   noise(a)  Nz = EDC[a] / (N - a), V = 10 log10 Nz.  Nz = 0 (the tail is silent: there is no floor) ends the row with
 *             status 3 and knee = N, before anything is fitted;
 *   run(V)    ip = the first index of the largest P_i; iF = the first i >= ip with D_i < V + margin_db, or I; R = [ip, iF);
 *   fit(S)    least squares of D_i over x_i = t_i - t_(min S), the four sums and the slope a of mc_ir_decay's step 5,
 *             c = (sum y - a sum x) / |S|; the line meets V at t_(min S) + (V - c) / a.  Fewer than 2 intervals, or an a that
 *             is not a finite negative number, end the row with status 2 (no decay above the floor);
 *   status 1  (too short or silent) cap < 1 or E = EDC[o] = 0;
 *   first     w0 = min(window or floor(0.03 rate + 0.5), cap); V = noise(N - tail); fit(run(V)) over means(w0); tc = the crossing;
 *   interval  w = clamp(floor(-10 / (a per_decade) + 0.5), 1, cap), chosen once; means(w);
 *   rounds    exactly `rounds` times: a_n = min(max(ceil(tc + margin_db / -a), o), N - tail); V = noise(a_n); R = run(V);
 *             S = {i in R : D_i <= V + margin_db + span_db}, or R when that has fewer than 2 members; fit(S); tc_prev = tc,
 *             tc = the crossing.  No convergence test: slot 6 reports the last change instead.
 * rows[(3 g + s) 8 ..] = {E, Nz, knee tc (taps, fractional, may lie past N), T = -60 / (a rate) seconds, 10 log10(max P_i / Nz) dB,
 *   w, |tc - tc_prev|, status}; with status != 0 the row holds E, the status and status 3's knee, every other entry is NaN.
 * A clean exponential IR has a knee too, near its end: its last tail_fraction is noise by definition, however far down.  Look
 * at slot 4, the peak-to-noise ratio, before acting on a knee: a floor 150 dB under the peak is the end of the file, not hiss. */
#define MC_FLOOR_MAX_XOVERS 3
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_floor_query) = 64 */
    uint32_t rate;          /* the rate the stored taps are at, [8000, 384000] */
    uint32_t n_xovers;      /* X, 0 .. MC_FLOOR_MAX_XOVERS: 1 + (X ? X + 1 : 0) row groups */
    uint32_t window;        /* first averaging interval in taps; 0 = floor(0.03 rate + 0.5) */
    float xover_hz[MC_FLOOR_MAX_XOVERS]; /* as mc_ir_damp: finite, [10, 0.45 rate], strictly ascending */
    float onset_db;         /* as mc_decay_query; default -20 */
    uint64_t end;           /* as mc_decay_query */
    float tail_fraction;    /* (0, 0.5]; default 0.1: the last share of the analysed taps that always counts as noise */
    float margin_db;        /* [1, 30]; default 10 */
    float span_db;          /* [5, 60]; default 20 */
    uint32_t per_decade;    /* 1 .. 20; default 5: intervals per 10 dB of decay */
    uint32_t rounds;        /* 1 .. 16; default 5 */
    uint32_t reserved;      /* must be 0 */
} mc_floor_query;
/* rate 44100, no crossovers (xover_hz = {250, 2000, 8000}), window 0, onset -20, end 0, and the defaults above */
void mc_default_floor_query(mc_floor_query *q);
/* rows: [(1 + (X ? X + 1 : 0)) * 3 * 8]; info = {origin tap, taps analysed N}.  Checked in this order, all before the engine or
 * the device is touched (MC_ERR_ARG, the message names the field): the query field by field, the pointers, idx ("IR not
 * loaded").  MC_ERR_STATE in the single-transform form, which keeps no taps.  Threading, stream and the promise that nothing
 * the engine holds changes are mc_ir_decay's; two calls with the same query on the same IR return the same bits. */
int mc_ir_floor(mc_engine *e, uint64_t idx, const mc_floor_query *q, double *rows, uint64_t info[2]);

/* The echo density of a loaded IR, measured on the device: where the IR stops being separate reflections and becomes a
 * diffuse tail (the mixing time), by Abel and Huang's normalised echo density (AES 121, 2006).  It is what mc_ir_synth's
 * late_start and build_up, mc_ir_room.last and the knee of a tail on a rendered IR (mc_ir_tail_move_knee) are set by.  No
 * reference equivalent; single-engine.  The stored taps are only read; N and the origin o are those of mc_ir_decay's step 1.
 * Everything is in double.  H = half or floor(0.01 rate + 0.5); hop = the field or max(1, floor(H / 4)).
 *   weights   h_k = (1 + cos(pi k / (H + 1))) / 2, k = -H .. H, all positive (computed on the host into a table);
 *   centres   t_i = o + i hop, i = 0 .. I - 1, I = floor((N - 1 - o) / hop) + 1;
 *   window i  the taps tau in [max(t_i - H, 0), min(t_i + H, N - 1)]; taps before o belong to it;
 *   values    v_c[tau] = (double) x_c[tau] (decay_t60 ? exp2((double)((int64) tau - (int64) t_i) 3 log2(10) / decay_t60) : 1):
 *             the decay inside the window is undone relative to its centre.  Without that a fast decay pulls the density of
 *             a mixed field under 1 (0.97 for 60 dB over nine window lengths); mc_ir_decay's T30 times the rate is what to pass;
 *   sums      ws = sum of h over the window, S_c = sum of h v_c^2, sigma_L = sqrt(S_L / ws), sigma_R likewise,
 *             sigma_LR = sqrt((S_L + S_R) / (2 ws));
 *   counts    A_L = sum of h [|v_L| > sigma_L] (strictly greater), A_R likewise,
 *             A_LR = (sum of h [|v_L| > sigma_LR] + sum of h [|v_R| > sigma_LR]) / 2;
 *   density   eta_s[i] = A_s / (ws 0.31731050786291415), the constant being erfc(1 / sqrt 2), the share of Gaussian noise beyond
 *             one standard deviation: near 0 for a few isolated reflections, 1 for a fully mixed field.  A silent window
 *             (sigma = 0) gives 0 through the strict comparison and is counted in slot 6;
 *   profile   profile[3 i + s] = eta_s[i], i < I; entries past I are not written;
 *   rows      from the profile in index order, i* = the first i with eta_s[i] >= threshold:
 *             rows[8 s ..] = {mixing tap t_(i*), mixing time (t_(i*) - o) / rate seconds, eta[0], max eta, tap of the first
 *             maximum, mean of eta over i >= i*, silent windows, status}; status 0: the threshold was reached; status 1: it
 *             never was, and slots 0, 1 and 5 are NaN. */
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_density_query) = 48 */
    uint32_t rate;          /* the rate the stored taps are at, [8000, 384000] */
    uint32_t half;          /* H: the window spans 2H + 1 taps; 0 = floor(0.01 rate + 0.5) (20 ms in all); else [4, 16384] */
    uint32_t hop;           /* taps between window centres; 0 = max(1, H / 4); else [1, 2^20] */
    float onset_db;         /* as mc_decay_query; default -20 */
    float threshold;        /* finite, (0, 2]; default 1 */
    uint64_t end;           /* as mc_decay_query */
    uint64_t decay_t60;     /* 0 = off; else the decay that is undone inside each window, in taps per 60 dB;
                               H 3 log2(10) / decay_t60 <= 256, so that v^2 can neither overflow nor vanish */
    uint32_t reserved[2];   /* must be 0 */
} mc_density_query;
/* rate 44100, half 0, hop 0, onset -20, threshold 1, end 0, decay_t60 0 */
void mc_default_density_query(mc_density_query *q);
/* rows: [3 * 8]; profile: [3 * Imax] with Imax = floor((N - 1) / hop) + 1, or NULL; info = {origin tap o, taps analysed N,
 * centres I}.  Checked in this order, all before the engine or the device is touched (MC_ERR_ARG, the message names the field):
 * the query field by field, the pointers, idx ("IR not loaded"), then the work bounds with o taken as 0: Imax <= 2^22 and
 * Imax (2H + 1) <= 2^34 (the message names hop).  MC_ERR_STATE in the single-transform form, which keeps no taps.  Threading,
 * stream and the promise that nothing the engine holds changes are mc_ir_decay's; two calls with the same query on the same
 * IR return the same bits. */
int mc_ir_density(mc_engine *e, uint64_t idx, const mc_density_query *q, double *rows, double *profile, uint64_t info[3]);

/* The interaural cross-correlation of a loaded IR, measured on the device (ISO 3382-1 Annex A): how alike the two channels
 * are, and at which lag.  It is the one readout of the relation between L and R: what mc_ir_synth.width and mc_ir_tail.width are
 * set by (mc_ir_tail_width_from_iacc), what tells how mc_ir_room.spacing came out, and what shows a swapped, delayed or
 * polarity-flipped channel of a captured pair.  No reference equivalent; single-engine.  The stored taps are only read.
 * Everything is in double.
 *   1. N and the origin o are those of mc_ir_decay's step 1; the row groups are those of its step 2: group 0 broadband,
 *      groups 1 .. n_bands the same two-section band-pass from rest at tap 0.  y_L and y_R are the group's doubles;
 *   2. windows: k = min(o + (split ? split : floor(0.08 rate + 0.5)), N); w = 0, 1, 2 are early [o, k), late [k, N), all [o, N);
 *   3. lags tau = -T .. T, T = max_lag (0 .. MC_IACC_MAX_LAG; 1 ms is floor(0.001 rate + 0.5));
 *   4. over a window [a, b): C_w(tau) = sum of y_L[m] y_R[m + tau] over the m with both m and m + tau inside [a, b);
 *      E_L,w = sum of y_L[m]^2 over [a, b), E_R,w likewise.  Both taps of a pair stay inside the window: C_w(tau) is then the
 *      inner product of two stretches of the window's own y_L and y_R, so |C_w(tau)| <= sqrt(E_L,w E_R,w) by Cauchy-Schwarz and
 *      |IACF| never exceeds 1, and the early figure holds nothing of the late field.  (A sum that let m + tau leave the window
 *      could exceed 1 for a short early window in front of a loud tail.);
 *   5. IACF_w(tau) = C_w(tau) / sqrt(E_L,w E_R,w); IACC_w = max over tau of |IACF_w(tau)|; tau* = the first lag, ascending
 *      from -T, that attains it.  A positive tau* means R is late: the sound came from the left;
 *   6. rows[(3 g + w) 8 ..] = {E_L, E_R, IACC, tau* (taps, signed), IACF(tau*) (signed: a negative value is a polarity flip),
 *      IACF(0), 10 log10(E_L / E_R) dB, status}.  Status 0: measured.  Status 1: the window is empty or E_L E_R = 0; slots 0, 1
 *      and 7 are set and the rest are NaN;
 *   7. curve[((3 g + w) (2T + 1)) + (tau + T)] = IACF_w(tau); a status-1 row's curve is NaN;
 *   8. info = {o, N, k}. */
#define MC_IACC_MAX_LAG 1024
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_iacc_query) = 88 */
    uint32_t rate;          /* the rate the stored taps are at, [8000, 384000] */
    uint32_t n_bands;       /* as mc_decay_query */
    uint32_t max_lag;       /* T, 0 .. MC_IACC_MAX_LAG taps */
    float centre_hz[MC_DECAY_MAX_BANDS]; /* as mc_decay_query */
    float q;                /* as mc_decay_query */
    float onset_db;         /* as mc_decay_query; default -20 */
    uint64_t end;           /* as mc_decay_query */
    uint64_t split;         /* taps from the origin to the late window; 0 = floor(0.08 rate + 0.5) (80 ms) */
    uint32_t reserved[2];   /* must be 0 */
} mc_iacc_query;
/* rate 44100, no bands, max_lag 44 (1 ms at that rate: set it again with the rate), q sqrt 2, onset -20, end 0, split 0 */
void mc_default_iacc_query(mc_iacc_query *q);
/* rows: [(1 + n_bands) * 3 * 8]; curve: [(1 + n_bands) * 3 * (2 max_lag + 1)] or NULL; info = {origin tap o, taps analysed N,
 * first late tap k}.  Checked in this order, all before the engine or the device is touched (MC_ERR_ARG, the message names the
 * field): the query (struct_size, rate, n_bands, max_lag, each used centre_hz, q, onset_db, reserved), the pointers, idx ("IR
 * not loaded"), then the work bounds: the lag products (1 + n_bands) N (2 max_lag + 1) <= 2^40, and the partial sums
 * 3 ceil(N / 2304) (2 max_lag + 3) <= 2^23 doubles (64 MiB of scratch; at max_lag 1024 that is 3.1 million taps, 65 s at 48 kHz); the message
 * names max_lag.  MC_ERR_STATE in the single-transform form, which keeps no taps.  Threading, stream and the promise that nothing
 * the engine holds changes are mc_ir_decay's; scratch is allocated by the call and freed before it returns; two calls with the
 * same query on the same IR return the same bits. */
int mc_ir_iacc(mc_engine *e, uint64_t idx, const mc_iacc_query *q, double *rows, double *curve, uint64_t info[3]);

/* The speech transmission index of a loaded IR, measured on the device: how well speech is understood through the room the
 * engine convolves with, from 0 (bad) to 1 (excellent).  It is obtained from the impulse response by Schroeder's relation (the
 * indirect method of IEC 60268-16): the modulation transfer function of the squared, octave-filtered response at n_mod
 * modulation frequencies in n_bands bands, folded into one number with the standard's band weights.  C50 and D50 of mc_ir_decay
 * are its coarse relatives.  No reference equivalent; single-engine.  The stored taps are only read.  Everything is in double,
 * computed from the fields as they are (floats, but for the weights).
 *   1. N and the origin o are those of mc_ir_decay's step 1; the row groups are those of its step 2: group 0 broadband,
 *      groups b = 1 .. n_bands the same two-section band-pass from rest at tap 0, at centre_hz[b - 1] with q.  y_L and y_R are
 *      the group's doubles;
 *   2. over the taps m in [o, N), for each channel c in {L, R} and each modulation frequency F_f = (double) mod_hz[f], f < n_mod,
 *      with theta = 2 pi F_f (m - o) / rate: C_c(f) = sum of y_c[m]^2 cos theta, S_c(f) = sum of y_c[m]^2 sin theta,
 *      E_c = sum of y_c[m]^2.  The channel sets s = 0, 1, 2 are L, R and L + R; the third set's C, S and E are the sums of the
 *      other two's (L + R), added after the taps have been summed: it is not walked again;
 *   3. m_s(f) = hypot(C, S) / E, the modulation transfer function.  With flags & MC_STI_SNR, in the band groups only, m is
 *      multiplied by 1 / (1 + 10^(-snr_db[b - 1] / 10)): stationary noise at that signal-to-noise ratio in band b.  A set with
 *      E = 0 or an E that is not finite has status 1, and its m and everything derived from it are NaN;
 *   4. the transmission index TI = 1 when m >= 1, 0 when m <= 0, else min(max((10 log10(m / (1 - m)) + 15) / 30, 0), 1): the
 *      apparent signal-to-noise ratio clipped to +/- 15 dB.  MTI = (sum of TI over f, ascending) / n_mod;
 *   5. STI_s = sum of alpha[b] MTI_b over the band groups (ascending b) less the sum of beta[b] sqrt(MTI_b MTI_(b+1)) over
 *      b < n_bands - 1 (ascending b, subtracted one by one after the alphas).  NaN when n_bands = 0 or a band of the set has
 *      status 1;
 *   6. mtf[((3 g + s) n_mod) + f] = m; rows[(3 g + s) 4 ..] = {E, MTI, status, 0}; sti[s]; info = {o, N}.
 * The standard's level-dependent auditory masking and its reception threshold need absolute sound pressure levels, which an
 * impulse response does not have: they are left out.  The default weights are IEC 60268-16's for male speech; a caller with
 * another set passes its own. */
#define MC_STI_MAX_BANDS 7
#define MC_STI_MAX_MOD 16
#define MC_STI_SNR 1u           /* flags: apply snr_db */
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_sti_query) = 272 (4 bytes of padding before end) */
    uint32_t rate;          /* the rate the stored taps are at, [8000, 384000] */
    uint32_t n_bands;       /* 0 .. MC_STI_MAX_BANDS */
    uint32_t n_mod;         /* 1 .. MC_STI_MAX_MOD */
    uint32_t flags;         /* MC_STI_SNR or 0; any other bit is refused */
    float centre_hz[MC_STI_MAX_BANDS];   /* as mc_decay_query: [10, 0.45 rate] */
    double alpha[MC_STI_MAX_BANDS];      /* the bands' weights: finite, >= 0.  Doubles, so that the defaults add up to 1 */
    double beta[MC_STI_MAX_BANDS - 1];   /* the redundancy of bands b and b + 1: finite, >= 0; the first n_bands - 1 are used */
    float snr_db[MC_STI_MAX_BANDS];      /* with MC_STI_SNR: finite, [-60, 120]; not looked at without */
    float mod_hz[MC_STI_MAX_MOD];        /* finite, [0.1, 50] */
    float q;                /* as mc_decay_query */
    float onset_db;         /* as mc_decay_query; default -20 */
    uint64_t end;           /* as mc_decay_query */
    uint32_t reserved[2];   /* must be 0 */
} mc_sti_query;
/* rate 44100, q sqrt 2, onset -20, end 0, no flag, snr_db 0; the seven octaves 125 .. 8000 Hz; the 14 modulation frequencies
 * 0.63, 0.8, 1, 1.25, 1.6, 2, 2.5, 3.15, 4, 5, 6.3, 8, 10, 12.5 Hz; alpha = 0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173 and
 * beta = 0.085, 0.078, 0.065, 0.011, 0.047, 0.095 (sum alpha - sum beta = 1).  A rate below 8000 / 0.45 Hz cannot hold the 8 kHz
 * octave: centre_hz[6] is then refused, and the caller passes fewer bands and weights of its own. */
void mc_default_sti_query(mc_sti_query *q);
/* rows: [(1 + n_bands) * 3 * 4]; mtf: [(1 + n_bands) * 3 * n_mod]; sti: [3]; info = {origin tap o, taps analysed N}.  Checked
 * in this order, all before the engine or the device is touched (MC_ERR_ARG, the message names the field): the query field by
 * field in struct order (struct_size, rate, n_bands, n_mod, flags, each used centre_hz, alpha, beta, snr_db under the flag,
 * mod_hz, q, onset_db, reserved), the pointers ("null rows", "null mtf", "null sti", "null info"), idx ("IR not loaded").
 * MC_ERR_STATE in the single-transform form, which keeps no taps.  Threading, stream and the promise that nothing the engine
 * holds changes are mc_ir_decay's; scratch is allocated by the call and freed before it returns; two calls with the same query
 * on the same IR return the same bits. */
int mc_ir_sti(mc_engine *e, uint64_t idx, const mc_sti_query *q, double *rows, double *mtf, double sti[3], uint64_t info[2]);

/* The frequency response of a loaded IR, measured on the device: the curve of the taps the engine convolves with, as every
 * convolution reverb shows it, at frequencies of the caller's choosing and over windows of the caller's choosing (one window:
 * the response; a row of overlapping windows: a waterfall).  mc_ir_eq_response and mc_ir_damp_response are the curves of the
 * filters a load applied; this is the curve of what came out.  No reference equivalent; single-engine.  The stored taps are only
 * read.  Everything is in double, computed from the fields as they are (frequencies are floats, as in every other query).
 *   1. N and the origin o are those of mc_ir_decay's step 1, from onset_db and end;
 *   2. window w covers the taps [a, b): a = min(o + first, N), b = count ? min(a + count, N) : N, L = b - a.  Its edges are
 *      raised cosines of r = min(rise, L) and f = min(fall, L - r) taps, the form of mc_ir_shape's fade: the weight of tap a + k
 *      is u = (1 - cos(pi (k + 1) / (r + 1))) / 2 for k < r, (1 + cos(pi (k' + 1) / (f + 1))) / 2 for the last f taps, k' counted
 *      from the first of them, and 1 between.  A window cannot be wrong: it clips, down to no taps at all.  win == NULL with
 *      n_win = 1 is the whole span, {0, 0, 0, 0};
 *   3. per channel c in {L, R} and frequency F_f = (double) hz[f], finite and in [0, rate / 2], with theta = 2 pi F_f (m - o) / rate
 *      and the sums over m in [a, b): H_c(f) = sum of u x_c[m] e^(-j theta), D_c(f) = sum of (m - o) u x_c[m] e^(-j theta),
 *      E_c = sum of (u x_c[m])^2, A_c = sum of |u x_c[m]|.  The phase of H is counted from the origin, not from tap 0;
 *   4. the group delay tau_c(f) = Re(D conj H) / |H|^2 in taps from o: exact, not a difference of phases.  NaN when |H|^2 is 0
 *      or not finite;
 *   5. status 1 when L = 0 or A is 0 or not finite: H = 0 and tau is NaN;
 *   6. resp[((2 w + c) n_freq + f) 3 ..] = {Re H, Im H, tau}; rows[(2 w + c) 4 ..] = {E, A, status, 0}; spans[2 w ..] = {a, b};
 *      info = {o, N}.
 * There is no third channel set: a mono sum's response is H_L + H_R and a power sum is |H_L|^2 + |H_R|^2, one line each for
 * the caller, and neither has an energy that is consistent with the other.  |delta H| <= (L + 227) 2^-53 A. */
#define MC_RSP_MAX_FREQ 1024
#define MC_RSP_MAX_WIN 64
typedef struct {
    uint64_t first;         /* the window's first tap, counted from the origin */
    uint64_t count;         /* its taps; 0: to the end of the span */
    uint32_t rise, fall;    /* the taps of its raised-cosine edges; clamped to the window */
} mc_response_window;       /* sizeof = 24 */
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_response_query) = 40 */
    uint32_t rate;          /* the rate the stored taps are at, [8000, 384000] */
    uint32_t n_freq;        /* 1 .. MC_RSP_MAX_FREQ */
    uint32_t n_win;         /* 1 .. MC_RSP_MAX_WIN */
    uint32_t flags;         /* must be 0 */
    float onset_db;         /* as mc_decay_query; default -20 */
    uint64_t end;           /* as mc_decay_query */
    uint32_t reserved[2];   /* must be 0 */
} mc_response_query;
/* rate 44100, n_freq 0 (the caller sets it with hz), n_win 1, onset -20, end 0 */
void mc_default_response_query(mc_response_query *q);
/* hz: [n_freq]; win: [n_win] or NULL (n_win = 1: the whole span); resp: [n_win * 2 * n_freq * 3]; rows: [n_win * 2 * 4]; spans:
 * [n_win * 2]; info = {origin tap o, taps analysed N}.  Checked in this order, all before the engine or the device is touched
 * (MC_ERR_ARG, the message names the field): the query field by field in struct order (struct_size, rate, n_freq - "n_freq 0
 * outside [1, 1024]" -, n_win, flags, onset_db, reserved), every hz[f], the pointers ("null hz", "null win" when n_win > 1, "null
 * resp", "null rows", "null spans", "null info"), idx ("IR not loaded").  MC_ERR_STATE in the single-transform form, which keeps
 * no taps.  Threading, stream and the promise that nothing the engine holds changes are mc_ir_decay's.  Scratch is the partial
 * sums of the largest window, ceil(L / 1024) (8 n_freq + 4) doubles, allocated by the call and freed before it returns.  Two
 * calls with the same query on the same IR return the same bits; a frequency's three numbers do not depend on the other
 * frequencies of the query or on its place among them, and a window's numbers do not depend on the other windows. */
int mc_ir_response(mc_engine *e, uint64_t idx, const mc_response_query *q, const float *hz, const mc_response_window *win,
                   double *resp, double *rows, uint64_t *spans, uint64_t info[2]);
/* Host arithmetic only.  hz[i] = (float)(lo_hz 2^(i / per_octave)), i = 0, 1, .. while that double is <= hi_hz: a grid with
 * per_octave points to the octave.  Returns the count; MC_ERR_ARG unless 0 < lo_hz <= hi_hz (finite), per_octave in [1, 96],
 * hz is not null and the count fits cap. */
int mc_response_grid(double lo_hz, double hi_hz, uint32_t per_octave, float *hz, uint32_t cap);
/* Host arithmetic only.  out[f] = the mean of power[g] over all g with hz[g] in [hz[f] 2^(-octaves / 2), hz[f] 2^(octaves / 2)],
 * summed in ascending g: fractional-octave smoothing of a power response (|H|^2) on any ascending grid.  hz [n]: finite, >= 0,
 * not descending; octaves finite in [0, 10]; with 0, out is power itself, bit for bit.  out may not overlap power. */
int mc_response_smooth(const float *hz, const double *power, uint32_t n, double octaves, double *out);

/* Synthesis of an IR on the device from a seed: a room from a few numbers instead of a recorded WAV.  No reference equivalent;
 * single-engine, as shaping is.  The F = frames stereo frames are generated at the session's rate into the buffer the shaped
 * load's steps read and never exist on the host.  Frame m is a pure function of (seed, m, this struct): the same struct gives
 * the same bits.
 *
 * Random words.  W(i, s) = Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; ten rounds)
 *   of the counter {i, 0, s, 0} under the key {seed & 0xffffffff, seed >> 32}: four 32-bit words w0 .. w3.
 *   u(w) = (w + 0.5) / 2^32 as double (exact, inside (0, 1)).
 * Late field.  For m >= late_start, t = m - late_start, from W(m, 0):
 *   gA = sqrt(-2 ln u(w0)) cos(2 pi u(w1)), gB = sqrt(-2 ln u(w2)) cos(2 pi u(w3)); rho = 1 - width (double from the float);
 *   L = gA, R = rho gA + sqrt(1 - rho^2) gB: width 0 gives R == L bit for bit, width 1 independent channels;
 *   envelope = late_gain * (t60 ? exp2(-(t 3 log2(10)) / t60) : 1), step 5's expression counted from late_start;
 *   echo density, with build_up = B > 0: the frame is occupied iff t + 1 >= B, or w0' < 2^28, or
 *   (uint64) w0' B^2 < ((uint64) (t + 1)^2) << 32, w0' = w0 of W(m, 1) - integer arithmetic only, so no rounding decides
 *   which frames sound.  The probability is p = t + 1 >= B ? 1 : max(1 / 16, ((t + 1) / B)^2); an occupied frame is scaled by
 *   1 / sqrt(p) (at most 4), an unoccupied one is exactly 0 in both channels: the expected energy follows the envelope whatever
 *   the density.  The late value is (L, R) * envelope * that scale.
 * Direct sound.  `direct` is added to both channels of frame 0.
 * Early reflections.  For j = 0 .. n_early - 1, from W(j, 2), with span = early_last - early_first + 1:
 *   pos = early_first + (((uint64) w0 span) >> 32) (integer arithmetic); g = early_gain (w1 & 1 ? -1 : 1) (early_first + 1) /
 *   (pos + 1); pan = width (2 u(w2) - 1); gL = g (pan >= 0 ? 1 - pan : 1), gR = g (pan <= 0 ? 1 + pan : 1) (the pan law of
 *   panDry / panWet).  Reflections with pos >= F are dropped; those that share a frame are added in ascending j.
 * A frame is late + direct + reflections, added in that order in double and rounded to float once. */
#define MC_SYNTH_MAX_EARLY 64
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_ir_synth) = 80 */
    uint32_t n_early;       /* 0 .. MC_SYNTH_MAX_EARLY */
    uint64_t seed;
    uint64_t frames;        /* F, 1 .. 2^24, at the session's rate */
    uint64_t late_start;    /* >= F: no late field */
    uint64_t t60;           /* 0 = no decay; else 60 dB down at frame late_start + t60 */
    uint32_t build_up;      /* 0 .. 65535; 0 = dense from late_start */
    float late_gain;        /* finite, >= 0: standard deviation of the late field at late_start */
    float direct, early_gain; /* finite */
    float width;            /* [0, 1] */
    uint32_t rate;          /* the session's rate, which mc_synth_ir's eq and damp need (the WAV loads take it as a parameter;
                               here it stands where a reserved word would): 0 = none, fine with no EQ band on and no damping;
                               else [8000, 384000] */
    uint64_t early_first, early_last; /* first <= last < 2^24, looked at when n_early > 0 */
} mc_ir_synth;
/* frames 0 (the caller's to set), seed 0, no reflections (early_gain 1, early_first = early_last = 0), late_start 0, t60 0,
 * build_up 0, late_gain 1, direct 0, width 1, rate 0 */
void mc_default_ir_synth(mc_ir_synth *s);
/* Generates the IR `synth` describes and stores it at idx as mc_load_ir_damped stores converted WAV frames: the generated
 * frames take their place at step 1 of the order of operations above, and shape, eq and damp (each may be NULL: off) apply
 * to them.  Checked in this order, all before the engine or the device is touched (MC_ERR_ARG, the message names the field,
 * the engine stays as it was): synth, field by field in the struct's order; damp (when on), eq and shape as by
 * mc_load_ir_damped with ir_rate = session_rate = synth->rate; then e, idx and nframes.  The frames always pass through the
 * shaping stage (the identity with everything off), so a synthesised IR counts as shaped: mc_ir_shape_info reports it with
 * out[0] = F; mc_ir_info, mc_ir_decay, fp16 storage and the single-transform form see the stored taps as after any shaped
 * load.  Threading as mc_load_ir. */
int mc_synth_ir(mc_engine *e, uint64_t idx, uint64_t nframes, const mc_ir_synth *synth, const mc_ir_shape *shape,
                const mc_ir_eq *eq, const mc_ir_damp *damp);
/* out = {frames generated (F), reflections kept (pos < F), first frame of the late field (min(late_start, F)), 0};
 * MC_ERR_STATE unless the IR's last load was mc_synth_ir */
int mc_ir_synth_info(const mc_engine *e, uint64_t idx, double out[4]);

/* Capture of an IR from a recorded exponential sine sweep (Farina's method): the sweep is played through a room, the
 * recording is deconvolved on the device with the sweep's inverse filter, and the result takes the place of a WAV's frames.
 * No reference equivalent; single-engine, as shaping is.
 *
 * The sweep.  N = frames; everything in double from the float fields:
 *   Ls = (N - 1) / ln(f2 / f1), so the instantaneous frequency is f1 at frame 0 and f2 at frame N - 1;
 *   phi(n) = (2 pi f1 Ls / rate) expm1(n / Ls);
 *   w(n) = the product of the fade-in window (1 - cos(pi (n + 1) / (fade_in + 1))) / 2 for n < fade_in and step 6's fade-out
 *   expression over the last fade_out frames: (1 + cos(pi (k + 1) / (fade_out + 1))) / 2, k = n - (N - fade_out);
 *   s[n] = amplitude w(n) sin(phi(n)).
 * The deconvolution weights.  u[j] = (4 f2 / (amplitude^2 Ls rate)) s64[j] exp(-(N - 1 - j) / Ls), s64 the unrounded sweep:
 *   the time-reversed sweep under Farina's 6 dB/octave envelope, folded into a correlation.  The constant is the
 *   stationary-phase value that makes |S U| = 1 inside the swept band (|S(f)|^2 ~ A^2 Ls / (4 f), f in cycles per sample), so
 *   the recovered IR has the level of the room whatever the amplitude.
 * The generated frames.  For c in {L, R} and m = 0 .. F - 1:
 *   h_c[m] = sum over j = 0 .. N - 1, ascending, of u[j] (double) r_c[m + j + offset], r = 0 outside [0, M);
 *   one double accumulator per output, updated by fma, rounded to float once.  The fixed order makes a frame a pure function
 *   of the inputs: the same bits whatever the grid.  A sweep recorded with no latency puts its direct sound at frame -offset;
 *   a negative offset keeps pre-roll, where the sweep's harmonic-distortion images land, for mc_ir_shape.start or the trim
 *   to cut. */
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_sweep) = 40 */
    uint32_t rate;          /* [8000, 384000]: the recording's rate and the session's, which eq and damp use */
    uint64_t frames;        /* N, 2 .. 2^22 */
    float f1_hz;            /* finite, >= 1 */
    float f2_hz;            /* finite, f1_hz < f2_hz <= 0.5 * rate */
    float amplitude;        /* finite, > 0 */
    uint32_t fade_in;       /* frames */
    uint32_t fade_out;      /* frames, fade_in + fade_out <= N */
    uint32_t reserved;      /* must be 0 */
} mc_sweep;
/* rate 44100, frames 0 (the caller's to set), 20 Hz .. 20000 Hz, amplitude 0.5 (WavFile's full scale is +-0.5, quirk Q5),
 * no fades */
void mc_default_sweep(mc_sweep *sw);
/* s[first .. first + count) rounded to float, mono.  Host arithmetic only: no engine and no HIP call.  MC_ERR_ARG for a bad
 * field (the message names it), a null pointer or first + count > N. */
int mc_sweep_generate(const mc_sweep *sw, float *out, uint64_t first, uint64_t count);
/* Deconvolves the recording lr (M = frames interleaved L,R frames at sweep->rate, 1 .. 2^24) into F = ir_frames (1 .. 2^24)
 * frames and stores them at idx as mc_load_ir_damped stores converted WAV frames: they take their place at step 1 of the
 * order of operations above, and shape, eq and damp (each may be NULL: off) apply to them.  offset lies in [-2^24, 2^24];
 * F * N <= 2^40, which bounds the one correlation launch.  Checked in this order, all before the engine or the device is
 * touched (MC_ERR_ARG, the message names the field, the engine stays as it was): sweep, field by field in the struct's order;
 * M, F, offset, F * N; damp (when on), eq and shape as by mc_load_ir_damped with ir_rate = session_rate = sweep->rate; then
 * lr, e, idx and nframes.  The frames always pass through the shaping stage, so the IR counts as shaped: mc_ir_shape_info
 * reports it with out[0] = F.  Threading as mc_load_ir. */
int mc_load_ir_sweep(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, const mc_sweep *sweep,
                     int64_t offset, uint64_t ir_frames, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp);
/* out = {N, M, F, offset}; MC_ERR_STATE unless the IR's last load was mc_load_ir_sweep */
int mc_ir_sweep_info(const mc_engine *e, uint64_t idx, double out[4]);

/* The tail step of an IR load (step 1a of the order of operations above): every frequency band of the F frames is cut at its
 * knee, or cross-faded there into decaying noise that continues the band's own slope at the band's own level (tail
 * extrapolation), which also lets a recording that stopped too early run out.  No reference equivalent; single-engine.  The
 * step sits before the selection, so a fade-out ends at the new last tap and decay_t60, damping and EQ act on the new tail.
 *
 * x = the F frames at the session's rate as double, frames at and past F reading as 0; F' = length ? length : F; X = n_xovers;
 * P_k(.) = crossover k's two identical HIGHCUT sections (mc_ir_damp's) from rest at frame 0 over [0, F').
 *   Fades.  Band j with K_j = knee[j] < F' is touched: W_j = min(fade, K_j); for m < K_j - W_j fo = 1, fi = 0; for
 *     K_j - W_j <= m < K_j theta = (pi / 2) (m - (K_j - W_j) + 1) / (W_j + 1), fo = cos theta, fi = sin theta; for m >= K_j
 *     fo = 0, fi = 1 (power-complementary: the two signals are uncorrelated).  A band with K_j >= F' is left alone: fo = 1,
 *     fi = 0 throughout.
 *   Noise (MC_TAIL_EXTEND).  v_L[m] = gA, v_R[m] = rho gA + sqrt(1 - rho^2) gB, rho = 1 - width, from the words W(m, 3) as
 *     mc_ir_synth's late field makes them from W(m, 0) (stream 3 is this step's own);
 *     g_j[m] = exp2(-((double)((int64) m - (int64) K_j) 3 log2(10)) / t60[j]);
 *     A_(j,c) = sqrt(10^(level_db[j][c] / 10) / beta_j), beta_j = the share of white noise band j passes: the mean over
 *     i = 0 .. 8191 of |B_j(e^(j pi (i + 0.5) / 8192))|^2, B_0 = H_1^2, B_j = H_(j+1)^2 - H_j^2, B_X = 1 - H_X^2, H_k one section's
 *     complex response (1 with X = 0), on the host in double; q_j[m] = fi_j A_(j,c) g_j where fi_j > 0, and 0 elsewhere.
 *   Output, per channel c, in double, rounded to float once:
 *     y[m] = fo_X x + sum over k = 1 .. X of (fo_(k-1) - fo_k) P_k(x) + [EXTEND] q_X v + sum over k of (q_(k-1) - q_k) P_k(v),
 *     added in that order: damping's rearrangement, twice.  With every fo = 1 the filters cancel, so frames before the first
 *     touched one, min over the touched bands of K_j - W_j, are the input's, bit for bit.  MC_TAIL_CUT is the same without the
 *     noise: each band fades to nothing at its knee, and mc_ir_shape.length shortens the IR. */
enum { MC_TAIL_OFF = 0, MC_TAIL_CUT = 1, MC_TAIL_EXTEND = 2 };
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_ir_tail) = 144 */
    uint32_t mode;          /* MC_TAIL_*; MC_TAIL_OFF: every other field ignored */
    uint32_t n_xovers;      /* X, 0 .. 3; 0 = one broadband band */
    float xover_hz[3];      /* the first X: finite, [10, 0.45 session_rate], strictly ascending */
    uint32_t fade;          /* W: cross-fade length in frames; the fade ends at the knee */
    float width;            /* [0, 1], as mc_ir_synth.width */
    uint64_t seed;
    uint64_t length;        /* F' = length ? length : F; 1 .. 2^24 */
    uint64_t knee[4];       /* K_j of band j = 0 .. X, a frame at the session's rate; >= F' leaves the band alone */
    uint64_t t60[4];        /* EXTEND, bands 0 .. X: > 0; band j's noise is 60 dB down t60[j] frames after K_j */
    float level_db[4][2];   /* EXTEND, bands 0 .. X: finite; 10 log10 of band j's power per frame at K_j, channel L, R */
} mc_ir_tail;
/* off; xover_hz = {250, 2000, 8000}; fade 0; width 1; seed 0; length 0; every knee UINT64_MAX; t60 1; levels 0 */
void mc_default_ir_tail(mc_ir_tail *t);
/* Fills n_xovers, xover_hz, knee, t60 and level_db of `tail` from a floor measurement (q, rows, info as mc_ir_floor took and
 * gave them); mode, seed, width, fade and length stay the caller's.  Host arithmetic only: no engine, no HIP call.  With
 * X >= 1 tail band j is read from row group j + 1, with X = 0 the one band from group 0: knee[j] = first + floor(tc) of the
 * group's L + R row, t60[j] = max(1, floor(T rate + 0.5)) of that row, level_db[j][c] = channel c's own row's line at that
 * knee, 10 log10 Nz_c + a_c (knee - first - tc_c) (from the L + R row less 10 log10 2 when the channel's row has a status).
 * A band whose L + R row has status != 0 or whose floor(tc) >= info[1] gets knee = UINT64_MAX and is left alone.  `first` is
 * mc_ir_shape_info's first kept frame when the measured load trimmed, else 0.  MC_ERR_ARG for a bad query or a null pointer. */
int mc_ir_tail_from_floor(const mc_floor_query *q, const double *rows, const uint64_t info[2], uint64_t first, mc_ir_tail *tail);
/* Moves band `band`'s knee to `frame` and slides both of its levels along the band's own line:
 * level_db[band][c] += 60 ((double) old knee - (double) frame) / t60[band], in double, rounded to float once.  It is how a
 * rendered or synthesised IR, which has no noise floor (Lundeby's knee lands near its last tap), gets its knee at the mixing
 * time mc_ir_density measured.  Host arithmetic only.  MC_ERR_ARG for a null tail or a struct_size mismatch, a mode other than
 * MC_TAIL_EXTEND, a band above n_xovers, or a band whose knee is UINT64_MAX (left alone by mc_ir_tail_from_floor). */
int mc_ir_tail_move_knee(mc_ir_tail *tail, uint32_t band, uint64_t frame);
/* Sets tail->width = (float) min(max(1 - rho, 0), 1): the width that continues an IR whose late broadband IACF(0)
 * (mc_ir_iacc's rows[(3 * 0 + 1) * 8 + 5]) is rho.  The tail's noise is v_R = rho gA + sqrt(1 - rho^2) gB with gA and gB independent
 * of unit variance, so its lag-0 coefficient E[v_L v_R] / sqrt(E[v_L^2] E[v_R^2]) = rho / sqrt(rho^2 + 1 - rho^2) is rho exactly:
 * a tail of width 1 - rho is as correlated as the field it takes over from.  A negative rho clamps to width 1 (independent
 * channels): the tail cannot be anti-correlated.  Host arithmetic only.  MC_ERR_ARG for a null tail, a struct_size mismatch or
 * a rho that is not finite; the tail is then unchanged. */
int mc_ir_tail_width_from_iacc(mc_ir_tail *tail, double rho);
/* mc_load_ir_damped with `tail` applied as step 1a.  With tail NULL or MC_TAIL_OFF the call is mc_load_ir_damped itself, bit for
 * bit.  With a tail on everything is checked before the engine or the device is touched (MC_ERR_ARG, the message names the
 * field, the engine stays as it was): tail field by field in the struct's order, then session_rate and ir_rate (both in [8000,
 * 384000]; 0 / 0 is refused because the crossovers need the session's rate) and F', then damp, eq and shape as by
 * mc_load_ir_damped.  Such a load counts as shaped: mc_ir_shape_info's out[0] is F'.  The same frames and structs store the
 * same bits. */
int mc_load_ir_tail(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate,
                    uint32_t session_rate, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp, const mc_ir_tail *tail);
/* mc_load_ir_sweep with `tail` applied to the deconvolved frames; tail NULL or MC_TAIL_OFF: mc_load_ir_sweep itself, bit for
 * bit.  With a tail on: tail field by field, then everything mc_load_ir_sweep checks, in its order, with F' after F. */
int mc_load_ir_sweep_tail(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, const mc_sweep *sweep,
                          int64_t offset, uint64_t ir_frames, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp,
                          const mc_ir_tail *tail);
/* out = {bands touched, F, F', first frame changed (F' when no band was touched)}; MC_ERR_STATE unless the IR's last load had
 * a tail on */
int mc_ir_tail_info(const mc_engine *e, uint64_t idx, double out[4]);

/* The phase step of an IR load (step 1b of the order of operations above): the frames are replaced by the minimum-phase impulse
 * response that has the same magnitude response.  An IR that carries acausal build-up or excess group delay adds that delay to
 * every note; trimming removes leading silence only.  The minimum-phase IR has its energy as early as its magnitude response
 * allows.  It is meant for short IRs (cabinets, equaliser captures); on a room it destroys the arrival times that make the room.
 * No reference equivalent; single-engine.  DESIGN.md 2.19 has the method (homomorphic, by the real cepstrum) and the reasons.
 *
 * Per channel, everything in double; x = the F frames the step takes (after steps 1 and 1a):
 *   Nfft = max(16, (smallest power of two >= F) << over_log2);
 *   X = FFT of x zero-padded to Nfft; p[k] = Re^2 + Im^2; pm = max p.  pm = 0: the channel's output is all zeros;
 *   p[k] = max(p[k], pm 10^(-floor_db / 10)) (the bins below it are the clamped bins); L[k] = ln(p[k]) / 2;
 *   c = Re IFFT(L), folded: c[0] and c[Nfft / 2] kept, c[1 .. Nfft / 2 - 1] doubled, the rest zero;
 *   C = FFT(c); Y[k] = exp(Re C) (cos Im C + i sin Im C); y = Re IFFT(Y);
 *   the step's output is y[0 .. F), rounded to float once.
 * The library carries both channels through one complex transform (L + i R), so a channel's bits depend on the other channel
 * below the last place of a double.  The same frames and struct store the same bits on every run.
 * floor_db bounds the dynamic range of the log spectrum: a deep notch would otherwise put a spike of ln(0) into it, whose
 * cepstrum does not fit Nfft / 2 and aliases.  The oversampling (2^over_log2) gives the cepstrum room to decay; 8 is the usual choice.
 * The output is truncated to F frames; mc_ir_phase_info tells how much energy that dropped.
 * Synthesised loads (mc_synth_ir and the room entry points) have no phase entry point. */
enum { MC_PHASE_OFF = 0, MC_PHASE_MINIMUM = 1 };
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_ir_phase) = 16 */
    uint32_t mode;          /* MC_PHASE_*; MC_PHASE_OFF: every other field ignored */
    float floor_db;         /* [40, 300]; default 120 */
    uint32_t over_log2;     /* 1 .. 6; default 3 (8 x) */
} mc_ir_phase;
/* off; floor_db 120; over_log2 3 */
void mc_default_ir_phase(mc_ir_phase *p);
/* What the step would do to `frames` frames, host arithmetic only: out = {Nfft, passes per transform (1 or 2), bytes of device
 * memory the step allocates while it runs, 0}.  MC_ERR_ARG for a null pointer, a field of `p` outside its range (mode
 * MC_PHASE_OFF is accepted and planned as if it were on), frames = 0 or frames and over_log2 beyond the limits below. */
int mc_ir_phase_plan(const mc_ir_phase *p, uint64_t frames, double out[4]);
/* mc_load_ir_tail with `phase` applied as step 1b.  With phase NULL or MC_PHASE_OFF the call is mc_load_ir_tail itself, bit for
 * bit, and leaves no phase information.  With the step on everything is checked before the engine or the device is touched
 * (MC_ERR_ARG, the message names the field, the engine stays as it was): phase field by field in the struct's order, then
 * everything mc_load_ir_tail checks, in its order; the step's limits, F <= 2^21 frames at the session's rate and Nfft <= 2^22
 * (the message names the frames or over_log2), come as soon as F is known: after the tail's F' with a tail on, else after
 * damp, eq, shape, the rates and the frames.  Without a tail the rates may be 0 / 0 as in mc_load_ir_shaped: the step does not
 * need the rate.  Such a load counts as shaped: mc_ir_shape_info's out[0] is F. */
int mc_load_ir_phase(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate,
                     uint32_t session_rate, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp, const mc_ir_tail *tail,
                     const mc_ir_phase *phase);
/* mc_load_ir_sweep_tail with `phase` applied to the deconvolved frames after the tail step; phase NULL or MC_PHASE_OFF:
 * mc_load_ir_sweep_tail itself, bit for bit.  With the step on: phase field by field, then everything mc_load_ir_sweep_tail
 * checks, in its order, with the step's limits after F (after F' with a tail on). */
int mc_load_ir_sweep_phase(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, const mc_sweep *sweep,
                           int64_t offset, uint64_t ir_frames, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp,
                           const mc_ir_tail *tail, const mc_ir_phase *phase);
/* out = {F, Nfft, E_in, E_out, Ts_in, Ts_out, clamped bins L, clamped bins R}: E = the sum over both channels of the squared
 * frames that went into and came out of the step (the output as stored, in float), Ts = sum m e[m] / sum e[m] with e[m] = L[m]^2 +
 * R[m]^2, the centre of energy in frames (0 when E = 0).  E_out / E_in is what the truncation to F frames kept, Ts_in - Ts_out
 * the delay removed.  The sums are made of one partial per 256 frames, added in ascending order.  MC_ERR_STATE unless the IR's
 * last load had the step on. */
int mc_ir_phase_info(const mc_engine *e, uint64_t idx, double out[8]);

/* The filter step of an IR load (step 1c of the order of operations above): the frames are combined with a second impulse
 * response, the filter.  Convolution cascades the two at load time - a cabinet into a room, a correction FIR into a hall - so
 * that the period and batch paths pay nothing for it.  Deconvolution divides the filter out of the frames: the response of the
 * playback and recording chain, as a loop-back capture gives it, out of a measured IR (Kirkeby's regularised inverse).
 * No reference equivalent; single-engine.  DESIGN.md 2.20 has the reasons.
 *
 * Per output channel c, everything in double; a_c = the F frames the step takes (after steps 1, 1a and 1b); the filter is G
 * stereo frames b at the session's rate (given at `rate` Hz, they are converted first as step 1 converts the IR, and G is
 * the count after that: ceil(filter_frames session / rate)):
 *   f_c = b_c (MC_FILTER_STEREO), b_L for both channels (MC_FILTER_LEFT) or (b_L + b_R) / 2 for both (MC_FILTER_MID);
 *   Nfft = max(16, smallest power of two >= F + G - 1); A = FFT of a_c zero-padded to Nfft, B = FFT of f_c likewise;
 *   MC_FILTER_CONVOLVE:   Y = A B;
 *   MC_FILTER_DECONVOLVE: p[k] = |B[k]|^2, pm = max p, eps = 10^(-reg_db / 10), Y = A conj(B) / (p + eps pm).  pm = 0: the
 *                         channel's output is all zeros.  The bins with p < eps pm are the regularised bins;
 *   y = Re IFFT(Y); the step's output is y[0 .. Fo), rounded to float once;
 *   Fo = frames_out when that is set, else F + G - 1 for a convolution (all of it) and F for a deconvolution.
 * The deconvolution is circular over Nfft points: what the inverse of the filter rings past Nfft comes back at the front.
 * The library carries both channels through one complex transform (L + i R), so a channel's bits depend on the other channel
 * below the last place of a double.  The same frames, filter and struct store the same bits on every run.
 * Synthesised loads (mc_synth_ir and the room entry points) have no filter entry point. */
enum { MC_FILTER_OFF = 0, MC_FILTER_CONVOLVE = 1, MC_FILTER_DECONVOLVE = 2 };
enum { MC_FILTER_STEREO = 0, MC_FILTER_LEFT = 1, MC_FILTER_MID = 2 };
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_ir_filter) = 32 */
    uint32_t op;            /* MC_FILTER_OFF / CONVOLVE / DECONVOLVE; MC_FILTER_OFF: every other field ignored */
    uint32_t channels;      /* MC_FILTER_STEREO / LEFT / MID */
    uint32_t rate;          /* Hz of the filter's frames, [8000, 384000]; 0 = the session's */
    float reg_db;           /* [20, 200]; default 60; read by a deconvolution only, checked always */
    uint32_t reserved;      /* must be 0 */
    uint64_t frames_out;    /* Fo; 0 = F + G - 1 (convolution) or F (deconvolution) */
} mc_ir_filter;
/* off; stereo; rate 0; reg_db 60; frames_out 0 */
void mc_default_ir_filter(mc_ir_filter *f);
/* What the step would do to `frames` frames with a filter of `filter_frames` frames, both at the session's rate (`rate` is
 * checked and not used), host arithmetic only: out = {Nfft, passes per transform (1 or 2), bytes of device memory the step
 * allocates while it runs (the filter's frames, the transforms' buffers and the partial sums), Fo}.  MC_ERR_ARG for a null
 * pointer, a field of `f` outside its range (MC_FILTER_OFF is planned as a convolution), frames = 0 or filter_frames = 0, or
 * lengths and frames_out beyond the limits below. */
int mc_ir_filter_plan(const mc_ir_filter *f, uint64_t frames, uint64_t filter_frames, double out[4]);
/* mc_load_ir_phase with `filter` applied as step 1c to the `filter_frames` interleaved stereo frames at filter_lr.  With filter
 * NULL or MC_FILTER_OFF the call is mc_load_ir_phase itself, bit for bit; it leaves no filter information and does not look at
 * filter_lr.  With the step on everything is checked before the engine or the device is touched (MC_ERR_ARG, the message names
 * the field, the engine stays as it was): filter field by field in the struct's order (frames_out apart), then everything
 * mc_load_ir_phase checks, in its order: phase, if it is on, field by field, then the tail, the rates and F' with a tail on, else
 * damp, eq, shape, the rates and the frames.  The step's limits come as soon as F is known, after the phase step's: a rate
 * that differs from a session_rate of 0 (the conversion needs the session's rate), filter_frames = 0 or above 2^40, Nfft <= 2^22
 * (the message names the frames) and frames_out, at most F + G - 1 for a convolution and Nfft for a deconvolution.  A null
 * filter_lr comes last, before the load's own null engine.  Such a load counts as shaped: mc_ir_shape_info's out[0] is Fo. */
int mc_load_ir_filter(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate,
                      uint32_t session_rate, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp, const mc_ir_tail *tail,
                      const mc_ir_phase *phase, const mc_ir_filter *filter, const float *filter_lr, uint64_t filter_frames);
/* mc_load_ir_sweep_phase with `filter` applied to the deconvolved frames after the phase step; the session's rate is the
 * sweep's.  filter NULL or MC_FILTER_OFF: mc_load_ir_sweep_phase itself, bit for bit.  With the step on: filter field by field,
 * then everything mc_load_ir_sweep_phase checks, in its order, with the step's limits after the phase step's, and a null
 * filter_lr after the null lr. */
int mc_load_ir_sweep_filter(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, const mc_sweep *sweep,
                            int64_t offset, uint64_t ir_frames, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp,
                            const mc_ir_tail *tail, const mc_ir_phase *phase, const mc_ir_filter *filter, const float *filter_lr,
                            uint64_t filter_frames);
/* out = {F, G, Fo, Nfft, E_in, E_filter, E_out, E_rest, regularised bins L, regularised bins R}: E_in = the sum over both
 * channels of the squared frames that went in, E_filter that of f_L and f_R (with LEFT and MID the one signal counts for
 * both channels), E_out that of the Fo frames as stored, in float, and E_rest that of y[Fo .. Nfft), in double, which the step
 * left behind: rounding noise after a whole convolution, the truncated tail or the wrapped-round ringing otherwise.  The bins
 * are 0 for a convolution.  The sums are made of one partial per 256 frames, added in ascending order.  MC_ERR_STATE unless
 * the IR's last load had the step on. */
int mc_ir_filter_info(const mc_engine *e, uint64_t idx, double out[10]);

/* The match step of an IR load (step 1d of the order of operations above): a match EQ.  The frames get the tonal balance of a
 * second impulse response, the target ("make this cabinet sound like that one"), or of a flat or tilted line.  The two
 * fractional-octave-smoothed power spectra are compared on a logarithmic grid, the difference is bounded and applied as a
 * short, smooth minimum-phase or linear-phase correction.  Unlike a deconvolution it leaves fine structure and phase alone,
 * and it changes tone, not level.  No reference equivalent; single-engine.  DESIGN.md 2.21 has the reasons.
 *
 * Per channel c, everything in double; a_c = the F frames the step takes (after steps 1 .. 1c); the target is G stereo frames
 * t at the session's rate `rate_s` (given at `rate` Hz, they are converted first as step 1 converts the IR, and G is the count
 * after that):
 *   Nfft = max(16, smallest power of two >= 2 max(F, G)); above 2^22 is refused.  A_c, T_c = the transforms of a_c and t_c
 *   zero-padded; Pa_c[k] = |A_c[k]|^2 and Pt_c[k] = |T_c[k]|^2 for k = 0 .. Nfft / 2;
 *   grid:    f_j = lo_hz 2^(j / per_octave) for j = 0, 1, .. while that double is <= hi_hz (mc_response_grid's rule): J points,
 *            2 <= J <= 1024;
 *   window:  k_lo = ceil(f_j 2^(-octaves / 2) Nfft / rate_s), k_hi = floor(f_j 2^(octaves / 2) Nfft / rate_s), both clipped to
 *            [1, Nfft / 2]; when k_lo > k_hi both are round-to-nearest(f_j Nfft / rate_s), clipped the same way;
 *   levels:  Sa_c[j] = the mean of Pa_c over the window, St_c[j] likewise; with MC_MATCH_FLAT there is no target and
 *            St_c[j] = 10^(tilt_db log2(f_j / 1000) / 10): tilt_db 0 whitens, -3 aims at pink.  With link the two channels'
 *            levels are added before anything else and one curve serves both channels, so the stereo image keeps its balance;
 *   floor:   S = max(S, max_j S 10^(-floor_db / 10)), for Sa and St separately.  A source channel whose frames are all zero is
 *            stored as zeros; when the source or the target of a curve is all zeros (of a linked curve: both channels) the
 *            curve is 0 dB throughout;
 *   curve:   raw[j] = 10 log10(St[j] / Sa[j]); m = the mean of raw, added in ascending j; d[j] = clamp(amount (raw[j] - m),
 *            -cut_db, +boost_db); a point counts as clamped when amount (raw[j] - m) lies outside that range;
 *   per bin, k = 0 .. Nfft / 2: u = per_octave log2(k rate_s / Nfft / lo_hz) clipped to [0, J - 1] (k = 0: u = 0),
 *            i = min(floor(u), J - 2), dB = d[i] + (u - i) (d[i + 1] - d[i]), L[k] = dB ln 10 / 20: flat outside [lo_hz, hi_hz];
 *   MC_MATCH_MINIMUM: the phase step's recipe on L mirrored to Nfft points: c = Re IFFT(L); c[0] and c[Nfft / 2] kept,
 *            c[1 .. Nfft / 2) doubled, the rest zero; C = exp(FFT(c)); Fo = F;
 *   MC_MATCH_LINEAR:  C[k] = exp(L[k]) e^(-2 pi i k D / Nfft), D = delay, the angle reduced as (k D mod Nfft) first;
 *            Fo = F + D, and F + D <= Nfft;
 *   Y_c = A_c C_c; y = Re IFFT(Y); the step's output is y[0 .. Fo), rounded to float once.
 * The step is circular over Nfft points.  The library carries both channels through one complex transform (L + i R), so a
 * channel's bits depend on the other channel below the last place of a double; every window's sum is made in an order that
 * depends on (k_lo, k_hi) alone.  The same frames, target and struct store the same bits on every run.
 * Synthesised loads (mc_synth_ir and the room entry points) have no match entry point. */
enum { MC_MATCH_OFF = 0, MC_MATCH_TARGET = 1, MC_MATCH_FLAT = 2 };
enum { MC_MATCH_MINIMUM = 0, MC_MATCH_LINEAR = 1 };
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_ir_match) = 80 */
    uint32_t mode;          /* MC_MATCH_OFF / TARGET / FLAT; MC_MATCH_OFF: every other field ignored */
    uint32_t phase;         /* MC_MATCH_MINIMUM / LINEAR */
    uint32_t link;          /* 0 or 1; default 1: one curve for both channels */
    uint32_t rate;          /* Hz of the target's frames, [8000, 384000]; 0 = the session's */
    uint32_t per_octave;    /* [1, 96]; default 12 */
    double lo_hz, hi_hz;    /* 1 <= lo_hz < hi_hz <= session rate / 2; default 20 and 0 = min(20000, session rate / 2) */
    double octaves;         /* the windows' width, [1/24, 2]; default 1/3 */
    float amount;           /* [0, 1]; default 1 */
    float boost_db, cut_db; /* [0, 60]; default 12 and 24 */
    float floor_db;         /* [40, 300]; default 120 */
    float tilt_db;          /* dB per octave of MC_MATCH_FLAT's line, [-12, 12]; default 0; checked always */
    uint32_t delay;         /* D of MC_MATCH_LINEAR in frames, <= 2^20; checked always */
    uint32_t reserved[2];   /* must be 0 */
} mc_ir_match;
/* off; minimum phase; linked; rate 0; 12 per octave from 20 Hz to min(20000, session rate / 2); a third of an octave; amount 1;
 * boost 12, cut 24, floor 120; tilt 0; delay 0 */
void mc_default_ir_match(mc_ir_match *m);
/* What the step would do to `frames` frames with a target of `target_frames` frames (ignored with MC_MATCH_FLAT), both at
 * session_rate Hz (`rate` is checked and not used), host arithmetic only: out = {Nfft, passes per transform (1 or 2), bytes of
 * device memory the step allocates while it runs, Fo, J, the sum of the J windows' widths in bins}.  MC_ERR_ARG for a null
 * pointer, a field of `m` outside its range (MC_MATCH_OFF is planned as MC_MATCH_TARGET), frames = 0, or the limits below. */
int mc_ir_match_plan(const mc_ir_match *m, uint64_t frames, uint64_t target_frames, uint32_t session_rate, double out[6]);
/* mc_load_ir_filter with `match` applied as step 1d, the target being the `target_frames` interleaved stereo frames at
 * target_lr.  With match NULL or MC_MATCH_OFF the call is mc_load_ir_filter itself, bit for bit; it leaves no match
 * information and does not look at target_lr.  With the step on everything is checked before the engine or the device is
 * touched (MC_ERR_ARG, the message names the field, the engine stays as it was): match field by field in the struct's order,
 * then everything mc_load_ir_filter checks, in its order.  The step's limits come as soon as F is known, after the filter
 * step's: a session_rate of 0 (the grid is in Hz), hi_hz above half the session's rate, J outside [2, 1024], target_frames = 0
 * (or above 2^40) with MC_MATCH_TARGET, Nfft above 2^22 (the message names the frames), F + delay above Nfft.  A null target_lr
 * with MC_MATCH_TARGET comes last, before the load's own null engine.  Such a load counts as shaped: mc_ir_shape_info's out[0]
 * is Fo. */
int mc_load_ir_match(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate,
                     uint32_t session_rate, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp, const mc_ir_tail *tail,
                     const mc_ir_phase *phase, const mc_ir_filter *filter, const float *filter_lr, uint64_t filter_frames,
                     const mc_ir_match *match, const float *target_lr, uint64_t target_frames);
/* mc_load_ir_sweep_filter with `match` applied to the deconvolved frames after the filter step; the session's rate is the
 * sweep's.  match NULL or MC_MATCH_OFF: mc_load_ir_sweep_filter itself, bit for bit.  With the step on: match field by field,
 * then everything mc_load_ir_sweep_filter checks, in its order, with the step's limits after the filter step's, and a null
 * target_lr after the null filter_lr. */
int mc_load_ir_sweep_match(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, const mc_sweep *sweep,
                           int64_t offset, uint64_t ir_frames, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp,
                           const mc_ir_tail *tail, const mc_ir_phase *phase, const mc_ir_filter *filter, const float *filter_lr,
                           uint64_t filter_frames, const mc_ir_match *match, const float *target_lr, uint64_t target_frames);
/* out = {F, G, Fo, Nfft, J, E_in, E_target, E_out, E_rest, mean removed L, mean removed R, clamped points}: G and E_target are
 * 0 with MC_MATCH_FLAT; E_in = the sum over both channels of the squared frames that went in, E_target that of the target's,
 * E_out that of the Fo frames as stored, in float, and E_rest that of y[Fo .. Nfft), in double, which the step left behind;
 * the means are m of either channel's curve in dB (the same number when linked); the clamped points are counted over the
 * curves there are, one when linked and two otherwise.  The sums are made of one partial per 256 frames, added in ascending
 * order.  MC_ERR_STATE unless the IR's last load had the step on. */
int mc_ir_match_info(const mc_engine *e, uint64_t idx, double out[12]);
/* The curve of IR idx's last load: hz[j] = f_j, before_db[2 j + c] = raw[j] - m and gain_db[2 j + c] = d[j] of channel c
 * (both channels hold the same numbers when linked), j < J.  Returns J; MC_ERR_ARG for a null pointer or cap < J (hz holds cap
 * numbers, before_db and gain_db 2 cap each); MC_ERR_STATE unless the IR's last load had the step on. */
int mc_ir_match_curve(const mc_engine *e, uint64_t idx, double *hz, double *before_db, double *gain_db, uint32_t cap);

/* The parts step of an IR load (step 1e of the order of operations above): the direct sound, the early reflections and the
 * late tail as three parts with controls of their own, as a convolution reverb offers them after "load".  The step is linear
 * in the taps, so it happens once at load time.  No reference equivalent; single-engine.  DESIGN.md 2.22 has the reasons.
 *
 * Positions are frames of the F frames that reach the step (after steps 1 .. 1d).  Part p = 0 is the direct sound, frames
 * before b_0 = direct_end; p = 1 the early reflections, from b_0 to b_1 = early_end; p = 2 the late tail, from b_1 on.  Either
 * boundary may lie past F, and the later parts are then empty.  Boundary k has a raised-cosine cross-fade of x_k = xfade[k]
 * frames around it that begins at s_k = b_k - floor(x_k / 2); s_0 >= 0 and s_0 + x_0 <= s_1 are required.  Weights of input
 * frame m (the shape's fade form), in double:
 *   u_k(m) = 0 for m < s_k, 1 for m >= s_k + x_k, else (1 - cos(pi (m - s_k + 1) / (x_k + 1))) / 2;
 *   w_0 = 1 - u_0, w_1 = u_0 - u_1, w_2 = u_1; x_k = 0 is a hard cut at b_k.
 * Coefficients of part p, made on the host in double from the struct's floats:
 *   g = 10^(gain_db / 20), negated when the part is inverted; a = (1 + width) / 2, b = (1 - width) / 2;
 *   gl = balance > 0 ? 1 - balance : 1, gr = balance < 0 ? 1 + balance : 1 (the synthesiser's pan law);
 *   c_LL = g gl a, c_LR = g gl b, c_RL = g gr b, c_RR = g gr a; when the part's input channels are swapped c_LL and c_LR change
 *   places, and c_RL and c_RR.
 * Output frame n, the parts that are not muted in the order p = 0, 1, 2, in double:
 *   m = n - delay_p, used when 0 <= m < F and w_p(m) > 0; t = w_p(m) x[m] per channel;
 *   acc_L += fma(c_LR, t_R, c_LL t_L); acc_R += fma(c_RL, t_L, c_RR t_R); the frame is (float) acc, rounded once.
 * Fo = frames_out when that is set, in [1, F + 2^24].  Otherwise Fo = the largest of (the end of part p's frames inside
 * [0, F)) + delay_p over the parts that are neither muted nor empty, where part 0 ends at min(F, s_0 + x_0), part 1 holds
 * [s_0, min(F, s_1 + x_1)) and part 2 [s_1, F).  Without such a part, or with that largest value <= 0, the load is refused.
 * Contributions that land outside [0, Fo) are dropped and reported.  Fo takes F's place in everything after the step.
 * Two consequences:
 *   - unity parts store the input's values: with gains of 0 dB, width 1, balance 0, no delay and no flag the stored values are
 *     the input's whatever the boundaries and the cross-fades (x w_0 + x w_1 + x w_2 in double lies within a few 2^-53 of the
 *     float x and rounds back to it; compared as values, -0 being +0);
 *   - width 0 stores equal channels bit for bit: fma(.5, R, .5 L) and fma(.5, L, .5 R) are the same rounded sum.
 * The onset search of step 2 sees the step's output: with the direct part muted and trim_db < 0 the trim moves to the first
 * reflection, which is then the caller's choice.  The same frames and struct store the same bits on every run.
 * Synthesised loads (mc_synth_ir and the room entry points) have no parts entry point: they have direct, reflection and late
 * gains of their own. */
enum { MC_PARTS_OFF = 0, MC_PARTS_ON = 1 };
#define MC_PARTS_MUTE(p) (1u << (p))         /* p = 0 direct, 1 early, 2 late */
#define MC_PARTS_SWAP(p) (1u << (4 + (p)))   /* the part's input channels change places */
#define MC_PARTS_INVERT(p) (1u << (8 + (p))) /* the part's sign */
typedef struct {
    uint32_t struct_size; /* sizeof(mc_ir_parts) = 104 */
    uint32_t mode;        /* MC_PARTS_OFF / ON; MC_PARTS_OFF: every other field ignored */
    uint32_t flags;       /* MC_PARTS_MUTE / SWAP / INVERT of p = 0, 1, 2; unknown bits: MC_ERR_ARG */
    uint32_t reserved0;   /* must be 0 */
    uint64_t direct_end;  /* b_0 <= 2^40 */
    uint64_t early_end;   /* b_1, b_0 <= b_1 <= 2^40 */
    uint32_t xfade[2];    /* x_0, x_1: b_0 >= floor(x_0 / 2) and s_0 + x_0 <= s_1 */
    int32_t delay[3];     /* frames, [-2^24, 2^24] */
    float gain_db[3];     /* [-120, 24] */
    float width[3];       /* [0, 2]: 0 mono, 1 as it is, 2 the side signal doubled */
    float balance[3];     /* [-1, 1]: -1 left only, +1 right only */
    uint64_t frames_out;  /* 0 = automatic; checked once F is known */
    uint32_t reserved[2]; /* must be 0 */
} mc_ir_parts;
/* off; no flag; both boundaries 0 (everything is the late part); no cross-fade; no delay; 0 dB; width 1; balance 0; automatic */
void mc_default_ir_parts(mc_ir_parts *p);
/* What the step would do to `frames` frames, host arithmetic only: out = {Fo, s_0, s_1, bytes of device memory the step
 * allocates while it runs}, coef[4 p + j] = c_LL, c_LR, c_RL, c_RR of part p.  MC_ERR_ARG for a null pointer, a field of `p`
 * outside its range (MC_PARTS_OFF is planned as MC_PARTS_ON), frames = 0, or the limits below. */
int mc_ir_parts_plan(const mc_ir_parts *p, uint64_t frames, double out[4], double coef[12]);
/* b_0 = onset + direct_frames and b_1 = onset + early_frames, everything else of `parts` left as it is: the counterpart of
 * mc_ir_tail_move_knee for an onset that mc_ir_shape_info or a measurement found.  Host arithmetic only.  MC_ERR_ARG for a null
 * parts, a struct_size mismatch, early_frames < direct_frames or a boundary above 2^40. */
int mc_ir_parts_at(mc_ir_parts *parts, uint64_t onset, uint64_t direct_frames, uint64_t early_frames);
/* mc_load_ir_match with `parts` applied as step 1e.  With parts NULL or MC_PARTS_OFF the call is mc_load_ir_match itself, bit
 * for bit; it leaves no parts information.  With the step on everything is checked before the engine or the device is touched
 * (MC_ERR_ARG, the message names the field, the engine stays as it was): parts field by field in the struct's order, then
 * everything mc_load_ir_match checks, in its order.  The step's limits come as soon as F is known, after the match step's:
 * frames_out above F + 2^24, and every part muted, empty or delayed to before frame 0.  Such a load counts as shaped:
 * mc_ir_shape_info's out[0] is Fo. */
int mc_load_ir_parts(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, uint32_t ir_rate,
                     uint32_t session_rate, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp, const mc_ir_tail *tail,
                     const mc_ir_phase *phase, const mc_ir_filter *filter, const float *filter_lr, uint64_t filter_frames,
                     const mc_ir_match *match, const float *target_lr, uint64_t target_frames, const mc_ir_parts *parts);
/* mc_load_ir_sweep_match with `parts` applied to the deconvolved frames after the match step.  parts NULL or MC_PARTS_OFF:
 * mc_load_ir_sweep_match itself, bit for bit.  With the step on: parts field by field, then everything mc_load_ir_sweep_match
 * checks, in its order, with the step's limits after the match step's. */
int mc_load_ir_sweep_parts(mc_engine *e, uint64_t idx, const float *lr, uint64_t frames, uint64_t nframes, const mc_sweep *sweep,
                           int64_t offset, uint64_t ir_frames, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp,
                           const mc_ir_tail *tail, const mc_ir_phase *phase, const mc_ir_filter *filter, const float *filter_lr,
                           uint64_t filter_frames, const mc_ir_match *match, const float *target_lr, uint64_t target_frames,
                           const mc_ir_parts *parts);
/* out = {F, Fo, b_0 clamped to F, b_1 clamped to F, E_direct, E_early, E_late, E_out, E_lost, contributions lost}: E_direct,
 * E_early and E_late = the sum over both channels of w_p(m)^2 x[m]^2 of part p, muted or not (so E_direct / (E_early + E_late)
 * is the IR's direct-to-reverberant ratio); E_out that of the Fo frames as stored, in float; E_lost that weighted energy of the
 * contributions of parts that are not muted which landed outside [0, Fo), and the last number how many there were.  The sums
 * are made of one partial per 256 frames, added in ascending order.  MC_ERR_STATE unless the IR's last load had the step on. */
int mc_ir_parts_info(const mc_engine *e, uint64_t idx, double out[10]);

/* The reflections of a rectangular room (Allen and Berkley's image-source method), added on the device to the frames
 * mc_ir_synth describes: the room itself - its size, where the source and the two receivers stand, how hard the walls are -
 * in place of reflections at random positions.  No reference equivalent; single-engine, as shaping is.  It gives the early
 * part of an IR; the tail step (mc_ir_floor, mc_ir_tail_from_floor, MC_TAIL_EXTEND) continues it at its own measured slope.
 *
 * Everything is computed in double from the float fields; rate = synth->rate, F = synth->frames, c = speed.
 * Receivers.  r_L = receiver - spacing / 2 and r_R = receiver + spacing / 2 along `axis`, the other coordinates the centre's.
 * Images.  For n = (n_x, n_y, n_z) in [-N, N]^3 and u in {0, 1}^3 the image lies at p_a = ((1 - 2 u_a) s_a + 2 n_a L_a) - r_a
 *   relative to a receiver r; d = sqrt(p_x^2 + p_y^2 + p_z^2);
 *   a = gain b_x b_y b_z / d, multiplied from the left, b_a = pow(beta_(a,0), |n_a - u_a|) pow(beta_(a,1), |n_a|), 0^0 = 1
 *   (beta_(a,0) is the wall at 0 of axis a, beta_(a,1) the wall at L_a); an image with a = 0 adds nothing;
 *   tau = d rate / c frames.  Each receiver (L, R) has its own p, d, a and tau.
 * Fractional delay.  k0 = floor(tau), f = tau - k0, s = sin(pi f).  For k = -15 .. 16, with x = k - f:
 *   w_k = (f == 0 ? (k == 0 ? 1 : 0) : (k odd ? s : -s) / (pi x)) (1 + cos(pi x / 16)) / 2, a Hann-windowed sinc over 16 zero
 *   crossings each side at the cost of one sine per image and channel.  An image whose delay is a whole number of frames is
 *   exactly one tap.
 * Which images sound.  E = last ? min(last, F) : F.  Channel c of an image is kept iff k0 < E; its tap k goes to frame
 *   m = k0 + k when 0 <= m < F, other taps are dropped.
 * Sum.  Each contribution is q = llrint(a w_k 2^40) (to nearest, ties to even), added into a 64-bit integer per frame and
 *   channel: integer sums do not depend on the order of arrival, so the same struct gives the same bits whatever the grid and
 *   however many images share a frame.  8 (2N + 1)^3 gain / min(d_direct,L, d_direct,R) must stay below 2^22, which excludes
 *   overflow: every image is farther away than the direct path, |beta| <= 1 and |w| <= 1 (and, with mc_ir_room_mics below,
 *   |gs gr| <= 1).
 * Frame.  (float)(late + direct + reflections + acc 2^-40), added in that order in double and rounded once; the first three
 *   terms are mc_ir_synth's.
 * Order 0.  N = ceil(E c / (rate 2 min(L))), refused above MC_ROOM_MAX_ORDER.  Every image with d < 2 N min(L) lies inside the
 *   lattice, because |p_a| >= 2 (|n_a| - 1) L_a: the lattice holds every image that arrives before frame E. */
#define MC_ROOM_MAX_ORDER 32
typedef struct {
    uint32_t struct_size;    /* sizeof(mc_ir_room) = 96 */
    uint32_t order;          /* N: lattice indices -N .. N per axis, at most MC_ROOM_MAX_ORDER; 0 = the smallest N whose lattice
                                is complete up to E */
    float size_m[3];         /* Lx, Ly, Lz: finite, [0.5, 200] */
    float source_m[3];       /* strictly inside the room */
    float receiver_m[3];     /* centre of the receiver pair, strictly inside the room */
    float beta[6];           /* pressure reflection coefficients of the walls x=0, x=Lx, y=0, y=Ly, z=0, z=Lz: [-1, 1] */
    float spacing_m;         /* finite, >= 0: the two omnidirectional receivers sit at receiver -/+ spacing / 2 along `axis`
                                (L, R), both strictly inside the room */
    uint32_t axis;           /* 0, 1, 2 */
    float speed;             /* c, m/s: finite, [100, 2000] */
    float gain;              /* amplitude of an image 1 m away: finite, (0, 16] */
    uint32_t reserved;       /* must be 0 */
    uint64_t last;           /* E = last ? min(last, F) : F: images arriving at or after frame E are left out */
} mc_ir_room;
/* 5 x 4 x 3 m, source (1, 1.5, 1.2), receiver (3.5, 2, 1.5), every beta 0.9, spacing 0.2, axis 0, speed 343, gain 1, order 0,
 * last 0 */
void mc_default_ir_room(mc_ir_room *r);
/* mc_synth_ir with the room's reflections added to the generated frames and `tail` applied to them as step 1a.  With room
 * NULL and tail NULL or MC_TAIL_OFF the call is mc_synth_ir itself, bit for bit; tail may be used without room.  Checked in
 * this order, all before the engine or the device is touched (MC_ERR_ARG, the message names the field, the engine stays as it
 * was): synth as by mc_synth_ir; room, field by field in the struct's order (the spacing is refused when it puts a receiver
 * outside the room), then synth->rate, which must be set ("the room needs the session's rate"), the two direct distances
 * (>= 0.1 m), the automatic order and the bound on the sum; tail as by mc_load_ir_tail, with F' after F; damp, eq and shape,
 * then e, idx and nframes as by mc_synth_ir. */
int mc_synth_ir_room(mc_engine *e, uint64_t idx, uint64_t nframes, const mc_ir_synth *synth, const mc_ir_room *room,
                     const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp, const mc_ir_tail *tail);
/* out = {N used, images kept L, images kept R (counted on the device), tau of the direct sound L, R (frames, fractional), E,
 * frames up to which the lattice is complete = floor(2 N min(L) rate / c), 0}; MC_ERR_STATE unless the IR's last load had a
 * room */
int mc_ir_room_info(const mc_engine *e, uint64_t idx, double out[8]);
/* What a load of `frames` frames at `rate` would do with `room`: out = {N that would be used, images in the lattice
 * 8 (2N + 1)^3, frames up to which it is complete, tau of the direct sound L, R, the volume (m^3), Sabine's and Eyring's
 * reverberation times (s)}.  The times come from the mean of 1 - beta^2 over the wall areas S: T = (24 ln 10 / c) V / (S abar)
 * and (24 ln 10 / c) V / (-S ln(1 - abar)); both are 0 when nothing absorbs.  They are estimates to compare against: the
 * method's own decay is slower than either, which is why a tail is measured (mc_ir_floor) and not computed.  The room is
 * checked as by mc_synth_ir_room, with rate in [8000, 384000] and frames in [1, 2^24].  Host arithmetic only: no engine and no
 * HIP call. */
int mc_ir_room_plan(const mc_ir_room *room, uint32_t rate, uint64_t frames, double out[8]);

/* Directional microphones and a directional source in the room of mc_ir_room: first-order patterns, which the image-source
 * method renders exactly.  An image source is the mirror of the real one, so its aim is mirrored with it; a receiver weighs
 * an arrival by the direction it comes from.  Only the amplitude of an image changes.  No reference equivalent.
 *
 * Aims.  Azimuth runs from +x towards +y, elevation towards +z, both in degrees; the unit vector of an aim is
 *   (cos el cos az, cos el sin az, sin el), computed on the host in double from the float fields: (double)deg * M_PI / 180.
 * Patterns.  A pattern is one number alpha in [0, 1], g(cos) = alpha + (1 - alpha) cos: 1 omni, 0.75 subcardioid, 0.5 cardioid,
 *   0.366 supercardioid, 0.25 hypercardioid, 0 figure-of-eight.  |g| <= 1, so the bound on the integer sum of mc_ir_room holds
 *   unchanged.
 * Receiver c sits where mc_ir_room puts it (spacing 0: a coincident pair), with its own pattern alpha_c and aim m_c.  For an
 *   image at p (from that receiver, as above), d = |p|: cr = (m_c . p) / d, gr = alpha_c + (1 - alpha_c) cr.
 * Source.  Pattern alpha_s, aim v.  The image (n, u) aims along v'_a = (1 - 2 u_a) v_a: mirrored on every axis it was reflected
 *   an odd number of times; translations do not turn it.  It radiates towards the receiver along -p: cs = -(v' . p) / d,
 *   gs = alpha_s + (1 - alpha_s) cs, per channel, since the two receivers see the image from different directions.
 * Amplitude.  a_c = (b / d_c) (gs_c gr_c), b = gain b_x b_y b_z as above.  The order is part of the definition: a dot product
 *   is fma(z, z', fma(y, y', x x')) and g is fma(1 - alpha, cos, alpha), which is exactly 1 for alpha = 1: omni microphones with
 *   an omni source store the bits of a room without microphones, and mirror-symmetric setups store equal channels.
 * Unchanged.  tau, k0, f, the keep rule k0 < E, the taps, the quantum, the one rounding, E, the accumulator and the automatic
 *   order.  The kept counts stay a matter of geometry: an image whose factor is 0 is counted, as one with b = 0 is.  A
 *   negative factor (the rear lobe of a figure-of-eight) is an ordinary negative contribution. */
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_ir_room_mics) = 48 */
    uint32_t flags;         /* must be 0 */
    float mic_pattern[2];   /* alpha of L, R: [0, 1] */
    float mic_az_deg[2];    /* finite, [-360, 360] */
    float mic_el_deg[2];    /* finite, [-90, 90] */
    float src_pattern;      /* [0, 1] */
    float src_az_deg, src_el_deg;   /* as the microphones' */
    uint32_t reserved;      /* must be 0 */
} mc_ir_room_mics;
/* every pattern 1 (omni), every angle 0 */
void mc_default_ir_room_mics(mc_ir_room_mics *m);
/* mc_synth_ir_room with `mics` in the room.  With mics NULL the call is mc_synth_ir_room itself, bit for bit.  mics without
 * room is MC_ERR_ARG ("the microphones need a room").  Checked in mc_synth_ir_room's order, the microphones field by field in
 * the struct's order right after the room and before the tail; the message names the field, nothing of the engine or the
 * device is touched before every check has passed, and the engine stays as it was on a refusal. */
int mc_synth_ir_room_mics(mc_engine *e, uint64_t idx, uint64_t nframes, const mc_ir_synth *synth, const mc_ir_room *room,
                          const mc_ir_room_mics *mics, const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp,
                          const mc_ir_tail *tail);
/* What `mics` do to the direct sound of `room`: out = {gs L, gs R, gr L, gr R, gs gr L, gs gr R, 0, 0}.  The room is checked
 * as by mc_ir_room_plan, then the microphones.  Host arithmetic only: no engine and no HIP call. */
int mc_ir_room_mics_plan(const mc_ir_room *room, const mc_ir_room_mics *mics, uint32_t rate, uint64_t frames, double out[8]);
/* The same eight numbers of the IR's last load; MC_ERR_STATE unless that load had microphones (mc_ir_room_info still answers
 * for a room without them) */
int mc_ir_room_mics_info(const mc_engine *e, uint64_t idx, double out[8]);

/* Walls and air that differ per frequency band in the room of mc_ir_room: carpet, curtains, glass and air take the highs
 * faster than the lows.  The room is rendered once per band with that band's walls and air loss, and the renderings are
 * joined by mc_ir_damp's band split, whose bands sum to their input exactly: no filter per image.  No reference equivalent.
 *
 * Bands.  X = n_xovers crossovers cut B = X + 1 bands, low to high; crossover k = 1 .. X is mc_ir_damp's: two identical
 *   high-cut sections at xover_hz[k - 1], q = 0.70710678f, at rate = synth->rate.
 * Band rendering.  Band j = 0 .. X is the room of mc_ir_room (and of mc_ir_room_mics when given) with beta[j] in place of
 *   room->beta and with each channel's amplitude multiplied by the air factor exp2(-(d_c k_j)),
 *   k_j = (double)air_db_per_m[j] * log2(10) / 20, made on the host: a_c = ((b / d_c) air_c) (gs_c gr_c), in that order.  Where
 *   air_db_per_m[j] == 0 no factor is applied at all: that band's rendering is mc_ir_room's, bit for bit.  tau, k0, f, the keep
 *   rule, the taps, the quantum 2^-40, E, A = min(E + 16, F), the automatic order and the kept counts (geometry only) are the
 *   room's and the same in every band.  Each band has its own 64-bit accumulator acc_j[A][2]; the bound on the integer sum
 *   holds per band, because the air factor is <= 1.
 * The join.  For k = 1 .. X: D_k[m] = (double)(acc_(k-1)[m] - acc_k[m]) 2^-40 for m < A and 0 for A <= m < F, the difference taken
 *   in int64 (both terms lie inside 2^62) and converted once (exact below 2^53, which every allowed room stays);
 *   P_k = D_k through crossover k's two sections from rest at frame 0 over all F frames: the ringing past the accumulator
 *   belongs to the IR;
 *   r[m] = (P_1[m] + .. + P_X[m]) + (m < A ? (double)acc_X[m] 2^-40 : 0), added low to high, the accumulator's term last.
 *   This is sum_j B_j(acc_j) over mc_ir_damp's bands B_0 = P_1, B_j = P_(j+1) - P_j, B_X = x - P_X, written by its differences.
 * Frame.  (float)(late + direct + reflections + r), rounded once.
 * Equal bands.  With X = 0, or with every D_k identically zero, every P_k is +0.0 and r is mc_ir_room's term: a banded room whose
 *   bands are all alike (and without air) stores the bits of the unbanded room.
 * With bands, room->beta is still checked as before but is not used for rendering. */
typedef struct {
    uint32_t struct_size;                          /* sizeof(mc_ir_room_bands) = 140 */
    uint32_t n_xovers;                             /* X: 0 .. MC_DAMP_MAX_XOVERS */
    float xover_hz[MC_DAMP_MAX_XOVERS];            /* the first n_xovers: finite, [10, 0.45 synth->rate], strictly ascending */
    float beta[MC_DAMP_MAX_XOVERS + 1][6];         /* band j = 0 .. n_xovers: the six walls in mc_ir_room's order, [-1, 1] */
    float air_db_per_m[MC_DAMP_MAX_XOVERS + 1];    /* band j: the air's loss in dB per metre, finite, [0, 1] */
    uint32_t flags;                                /* must be 0 */
    uint32_t reserved;                             /* must be 0 */
} mc_ir_room_bands;
/* n_xovers 0 (one band), every beta 0.9, no air loss */
void mc_default_ir_room_bands(mc_ir_room_bands *b);
/* mc_synth_ir_room_mics with `bands` in the room.  With bands NULL the call is mc_synth_ir_room_mics itself, bit for bit.
 * bands without room is MC_ERR_ARG ("the bands need a room").  Checked in mc_synth_ir_room_mics' order, the bands field by
 * field in the struct's order right after the microphones and before the tail (entries of the bands in use; the crossovers
 * against synth->rate); the message names the field, nothing of the engine or the device is touched before every check has
 * passed, and the engine stays as it was on a refusal. */
int mc_synth_ir_room_bands(mc_engine *e, uint64_t idx, uint64_t nframes, const mc_ir_synth *synth, const mc_ir_room *room,
                           const mc_ir_room_mics *mics, const mc_ir_room_bands *bands, const mc_ir_shape *shape, const mc_ir_eq *eq,
                           const mc_ir_damp *damp, const mc_ir_tail *tail);
/* What a load of `frames` frames at `rate` would do with `bands` in `room`: out[0] = B; out[1..3] = the crossovers (Hz; unused
 * ones 0); out[4..7] = Sabine's and out[8..11] = Eyring's reverberation time per band (s; unused bands 0), mc_ir_room_plan's
 * formulas on beta[j] with 4 m_j V added to the absorption area S abar and to -S ln(1 - abar), m_j = air_db_per_m[j] ln(10) / 10
 * the air's energy loss in nepers per metre; a time is 0 when nothing absorbs; out[12..15] = 0.  The room is checked as by
 * mc_ir_room_plan, then the bands.  Host arithmetic only: no engine and no HIP call. */
int mc_ir_room_bands_plan(const mc_ir_room *room, const mc_ir_room_bands *bands, uint32_t rate, uint64_t frames, double out[16]);
/* The same sixteen numbers of the IR's last load; MC_ERR_STATE unless that load had bands (mc_ir_room_info and
 * mc_ir_room_mics_info still answer for such a load) */
int mc_ir_room_bands_info(const mc_engine *e, uint64_t idx, double out[16]);

/* A binaural listener in the room of mc_ir_room: a rigid sphere in place of the receiver pair, by Brown and Duda's structural
 * model (IEEE Trans. Speech Audio Proc. 6(5), 1998).  Each ear hears an arrival with a delay that depends on its direction
 * (Woodworth's path around the sphere) and through a first-order head-shadow shelf: up to +6 dB towards the ear, down to about
 * -20 dB behind the head at high frequencies, unity at DC.  The shelf is
 * H(s, theta) = (1 + alpha(theta) s / wc) / (1 + s / wc) = 1 + (alpha(theta) - 1) HP(s) with HP one fixed first-order
 * high-pass: no filter per image, but two accumulators, a plain one and one that goes through HP once.  No reference equivalent.
 * Limits: a far-field model (no dependence on range), no pinna, no torso and no elevation cue beyond the cone of confusion the
 * sphere leaves, and the head is upright.
 *
 * Everything is computed in double from the float fields; rate = synth->rate, c = room->speed, a = radius_m.
 * Head.  The centre is room->receiver_m, and both ears are rendered from the centre; room->spacing_m and axis are checked as
 *   before but not used, as room->beta is with bands.  The head is upright: az = facing_az_deg and ear = ear_deg, both
 *   (double)deg * M_PI / 180, azimuth from +x towards +y as for the microphones; the ear axes, made on the host, are
 *   e_L = (cos(az + ear), sin(az + ear), 0) and e_R = (cos(az - ear), sin(az - ear), 0).
 * Per image and ear c.  p is the image's position relative to the centre as in mc_ir_room, d = |p|, once for both ears;
 *   cs_c = min(1, max(-1, (e_c . p) / d)), the dot product fma(z, z', fma(y, y', x x')) as for the microphones; th_c = acos(cs_c).
 * Delay.  g_c = cs_c >= 0 ? -cs_c : th_c - pi / 2: the plane wave's path to a point on a sphere, shorter by up to a on the near
 *   side, around the sphere on the far side, continuous at 90 degrees.  tau_c = fma(a, g_c, d) * rate / c.  k0, f, the 32 taps and
 *   the keep rule k0 < E are the room's, per ear.
 * Shadow.  h_c = shadow * fma(0.95, cos(1.2 * th_c), 0.05): Brown and Duda's alpha - 1 with alpha_min = 0.1 and theta_min = 150
 *   degrees, in [-0.9, 1] times shadow.
 * Amplitude.  a_c is the room's: b / d, times the band's air factor, times the source's factor gs_c when mics is given (with a
 *   head mics->mic_pattern[] must both be 1: ears are not microphones; the source's pattern and aim apply as before).  The
 *   shadow amplitude is s_c = a_c h_c.
 * Sums.  qP = llrint(a_c w_k 2^40) goes into accP[k0 + k][c] and qS = llrint(s_c w_k 2^40) into accS[k0 + k][c], both int64 [A][2],
 *   A = min(E + 16, F).  The room's bound on the sum covers both, because |h| <= 1.
 * The shelf's fixed part.  K = tan(c / (a rate)): the corner wc = 2 c / a rad/s, prewarped.  b0 = 1 / (1 + K), b1 = -b0,
 *   a1 = -(1 - K) / (1 + K); y = b0 v + s, s' = b1 v - a1 y: the first section of mc_ir_damp's crossover step with b2 = a2 = 0, one
 *   state per channel, from rest at frame 0 over all F frames on v[m] = accS[m] 2^-40 for m < A (converted once) and 0 from
 *   there.  The ringing past A belongs to the IR.
 * Term.  r[m] = S[m] + (m < A ? accP[m] 2^-40 : 0), the shelf's output S first.
 * Frame.  (float)(late + direct + reflections + r), rounded once.
 * With bands.  Each band renders its own accP_j and accS_j; mc_ir_room_bands' join is applied to the accP_j, giving rP [F], and
 *   separately to the accS_j, giving rS [F] (with X = 0 the join is the one accumulator's values); r = HP(rS) + rP in the order
 *   above.  Equal bands without air store the bits of the unbanded room with the same head.
 * Order and completeness.  An image outside the lattice has d >= 2 N min(L) and can arrive up to a / c earlier than d / c: with
 *   a head, complete = floor((2 N min(L) - a) rate / c), and order 0 picks the smallest N with complete >= E.  mc_ir_room_info
 *   reports these and the ears' direct delays for such a load.
 * shadow 0 leaves the pure delays: accS stays zero, S is +0.0 everywhere and r is accP's term. */
typedef struct {
    uint32_t struct_size;   /* sizeof(mc_ir_room_head) = 32 */
    uint32_t flags;         /* must be 0 */
    float radius_m;         /* a: finite, [0.05, 0.15] */
    float facing_az_deg;    /* finite, [-360, 360] */
    float ear_deg;          /* the ears' angle from the facing direction: finite, [60, 120]; Brown and Duda place them at 100 */
    float shadow;           /* [0, 1]: the depth of the shelf, 0 = delays only */
    uint32_t reserved[2];   /* must be 0 */
} mc_ir_room_head;
/* radius 0.0875 m, facing 0, ears at 90 degrees, shadow 1 */
void mc_default_ir_room_head(mc_ir_room_head *h);
/* mc_synth_ir_room_bands with `head` as the room's receiver.  With head NULL the call is mc_synth_ir_room_bands itself, bit for
 * bit.  head without room is MC_ERR_ARG ("the head needs a room").  Checked in mc_synth_ir_room_bands' order, the head right
 * after the bands and before the tail: radius_m, facing_az_deg, ear_deg, shadow, flags, reserved; then c / (a rate) < 1.5 ("the
 * head's corner lies above the rate"), the direct distance from the centre (>= a + 0.1 m), the automatic order and the bound on
 * the sum with the head's order, and mics->mic_pattern[], which must both be 1.  The message names the field, nothing of the
 * engine or the device is touched before every check has passed, and the engine stays as it was on a refusal. */
int mc_synth_ir_room_head(mc_engine *e, uint64_t idx, uint64_t nframes, const mc_ir_synth *synth, const mc_ir_room *room,
                          const mc_ir_room_mics *mics, const mc_ir_room_bands *bands, const mc_ir_room_head *head,
                          const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp, const mc_ir_tail *tail);
/* What a load of `frames` frames at `rate` would do with `head` in `room`: out = {N, complete, tau L, tau R of the direct sound
 * (frames), ITD = (tau R - tau L) / rate (s), theta L, theta R of the direct sound (degrees), h L, h R, the shelf's corner
 * c / (pi a) (Hz), K, 0}.  The room is checked as by mc_ir_room_plan, then the head.  Host arithmetic only: no engine and no HIP
 * call. */
int mc_ir_room_head_plan(const mc_ir_room *room, const mc_ir_room_head *head, uint32_t rate, uint64_t frames, double out[12]);
/* The same twelve numbers of the IR's last load; MC_ERR_STATE unless that load had a head */
int mc_ir_room_head_info(const mc_engine *e, uint64_t idx, double out[12]);

/* A plate reverberator (a thin steel sheet, a driver and two pickups: the EMT 140), added on the device to the frames
 * mc_ir_synth describes as the sum of the modes of a simply supported rectangular plate.  A plate is not a room: its modal
 * density is constant over frequency, so it is dense from the first millisecond, it is dispersive, and its decay falls with
 * frequency.  No reference equivalent; single-engine and load-time only, as shaping is.
 *
 * Everything is computed in double from the float fields; rate = synth->rate, F = synth->frames.
 * Plate.  Sides Lx, Ly = size_m (metres), thickness h = thickness_mm / 1000, Young's modulus E = young_gpa 10^9, density rho,
 *   Poisson's ratio nu.  Stiffness kappa = sqrt(E h^2 / (12 rho (1 - nu^2))) in m^2/s.
 * Modes.  For m, n >= 1 mode (m, n) has f_mn = (pi kappa / 2) ((m / Lx)^2 + (n / Ly)^2) Hz and the shape
 *   Phi_mn(x, y) = sin(m pi x / Lx) sin(n pi y / Ly).  Those with low_hz <= f_mn <= high_hz are kept, enumerated with m ascending
 *   and n ascending within each m: the row order of the mode table.  M is the number kept; M = 0 and M above
 *   MC_PLATE_MAX_MODES are refused.  high_hz must lie below rate / 2; 0 stands for min(20000, 0.45 rate).
 * Loss.  s_i = t60_s[i] ? 3 ln 10 / t60_s[i] : 0 per second: t60_s[0] is the decay time towards 0 Hz, t60_s[1] the one at
 *   damp_hz, 0 is no loss at that end.  sigma(f) = s_0 + (s_1 - s_0) f / damp_hz: Bilbao's two-parameter loss
 *   sigma_0 + sigma_1 k^2, which is linear in f because omega = kappa k^2.  s_1 >= s_0 is required (the highs decay no slower
 *   than the lows).  The damped frequency is taken as f_mn; low_hz >= 1 keeps sigma far below omega.
 * Amplitudes.  The driver sits at driver_m, pickup c = L, R at pickup_m[c], all strictly inside the plate:
 *   a_jc = gain 4 sqrt(2 / M) Phi_j(driver) Phi_j(pickup c).  The mean square of Phi Phi is 1/16 and M cosines of random
 *   phase add in power, so the expected RMS of the first milliseconds is `gain`.
 * Term.  With E = last ? min(last, F) : F, for frames t < E
 *   y_c[t] = sum_j a_jc exp(-sigma_j t / rate) cos(2 pi frac(nu_j t)), nu_j = f_j / rate,
 *   the phase reduced in turns, not in radians.
 * Evaluation.  exp cos at (j, t) is a pure function of row j of the table and t, whatever the launch, F and M: frames come in
 *   groups of MC_PLATE_GROUP aligned to multiples of it.  At a group's first frame t0 the value is z = exp(-(sigma_j / rate) t0)
 *   (cos, sin)(2 pi (nu_j t0 - rint(nu_j t0))), the difference made with one fused multiply-add; each later frame of the group
 *   is the one before times r_j = exp(-sigma_j / rate) (cos, sin)(2 pi nu_j) as complex numbers, and exp cos is the real part.
 * Sum.  mc_ir_room's rule: each contribution is q = llrint(a_jc exp cos 2^40) (to nearest, ties to even), added into a 64-bit
 *   integer per frame and channel, so the same struct stores the same bits whatever the grid.  gain 4 sqrt(2 M) must stay
 *   below 2^22, which excludes overflow.
 * Frame.  (float)(late + direct + reflections + acc 2^-40), added in that order in double and rounded once; the first three
 *   terms are mc_ir_synth's.
 * Work.  E M, the (mode, frame) pairs, may not exceed MC_PLATE_MAX_PAIRS. */
#define MC_PLATE_MAX_MODES 262144       /* 2^18 */
#define MC_PLATE_GROUP 32               /* K: frames per aligned group of the evaluation rule */
#define MC_PLATE_SLAB 256               /* rows of the mode table a workgroup stages at a time */
#define MC_PLATE_MAX_PAIRS 68719476736  /* 2^36 */
typedef struct {
    uint32_t struct_size;    /* sizeof(mc_ir_plate) = 88 */
    float size_m[2];         /* Lx, Ly: finite, [0.05, 10] */
    float thickness_mm;      /* finite, [0.05, 50] */
    float young_gpa;         /* finite, [0.1, 2000] */
    float density;           /* kg/m^3: finite, [100, 30000] */
    float poisson;           /* [0, 0.499] */
    float driver_m[2];       /* strictly inside the plate */
    float pickup_m[2][2];    /* pickup L (x, y), pickup R (x, y): strictly inside the plate */
    float low_hz;            /* finite, [1, 100000] */
    float high_hz;           /* 0 = min(20000, 0.45 rate); else finite, above low_hz and below rate / 2 */
    float t60_s[2];          /* seconds towards 0 Hz and at damp_hz: 0 (no loss) or finite in [0.001, 1000]; s_1 >= s_0 */
    float damp_hz;           /* finite, [10, 1000000] */
    float gain;              /* finite, (0, 16] */
    uint32_t reserved;       /* must be 0 */
    uint64_t last;           /* E = last ? min(last, F) : F: frames at and after E get nothing from the plate */
} mc_ir_plate;
/* steel (200 GPa, 7850 kg/m^3, 0.3), 0.5 mm, 2.04 x 0.97 m (sides whose squares are in no rational ratio: exactly 2 x 1 m makes
 * many modes coincide; commensurate sides stay legal), driver (0.83, 0.41), pickups (0.31, 0.67) and (1.57, 0.29), off every
 * low-order nodal line, low_hz 20, high_hz 0, t60 4 s at 0 Hz and 1 s at damp_hz 10000, gain 1, last 0 */
void mc_default_ir_plate(mc_ir_plate *p);
/* mc_synth_ir_room(..., room = NULL, ...) with the plate's term added to the generated frames; with plate NULL it is that call
 * bit for bit.  A plate and a room in one load are not offered.  Checked in this order, all before the engine or the device is
 * touched (MC_ERR_ARG, the message names the field, the engine stays as it was): synth as by mc_synth_ir; the plate field by
 * field in the struct's order; then synth->rate, which must be set ("the plate needs the session's rate"), high_hz below
 * rate / 2, M, the bound on the sum and the work cap (the message says by how much it is exceeded); tail as by mc_load_ir_tail,
 * with F' after F; damp, eq and shape, then e, idx and nframes as by mc_synth_ir_room. */
int mc_synth_ir_plate(mc_engine *e, uint64_t idx, uint64_t nframes, const mc_ir_synth *synth, const mc_ir_plate *plate,
                      const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp, const mc_ir_tail *tail);
/* What a load of `frames` frames at `rate` would do with `plate`: out = {M, the lowest and the highest kept mode (Hz), kappa
 * (m^2/s), Weyl's modal density Lx Ly / (2 kappa) (modes per Hz), T60 = 3 ln 10 / sigma at low_hz and at the highest kept mode
 * (s; 0 = no loss), the pairs E M}.  The plate is checked as by mc_synth_ir_plate, with rate in [8000, 384000] and frames in
 * [1, 2^24].  Host arithmetic only: no engine and no HIP call. */
int mc_ir_plate_plan(const mc_ir_plate *plate, uint32_t rate, uint64_t frames, double out[8]);
/* Rows first .. first + count - 1 of the mode table as {m, n, f (Hz), sigma (1/s), a_L, a_R} in double, six numbers a row: the
 * table a load uploads, made by the one function that makes it there.  first + count may not exceed M.  The plate is checked
 * as by mc_ir_plate_plan (the work cap aside: no frames are involved).  Host arithmetic only. */
int mc_ir_plate_modes(const mc_ir_plate *plate, uint32_t rate, uint64_t first, uint64_t count, double *rows);
/* out = {M, modes with a non-zero amplitude in L, in R, E, the lowest and the highest kept mode (Hz), kappa, 0}; MC_ERR_STATE
 * unless the IR's last load had a plate */
int mc_ir_plate_info(const mc_engine *e, uint64_t idx, double out[8]);

/* A spring reverberation tank (up to three helical springs between a driver and a pickup), added on the device to the frames
 * mc_ir_synth describes.  A spring is neither a room nor a plate: the helix is strongly dispersive, so every echo is a chirp
 * (below a transition frequency of a few kHz the lows arrive first and the highs tens of milliseconds later; a much weaker
 * second family of chirps lies above it), and the echoes repeat at the spring's round-trip time.  The model is the parametric
 * one of Valimaki, Parker and Abel (JAES 2010): a cascade of stretched all-pass sections in a feedback loop with a delay.  In
 * time that recursion is serial; as a transfer function it is closed form at every z, so the device evaluates it bin by bin,
 * transforms once and undoes a radius.  No reference equivalent; single-engine and load-time only, as shaping is.
 *
 * Everything is computed in double from the float fields; rate = synth->rate, F = synth->frames; round is to nearest, ties to
 * even.
 * Springs.  Spring s is present when delay_ms[s] != 0; the present ones come first, at least one is present, S is their count.
 *   Channel L uses the period T_s = delay_ms[s] / 1000, channel R T_s (1 + stereo).
 * Low chirps.  K = max(1, round(rate / (2 transition_hz))), at most MC_SPRING_MAX_STRETCH; f_t = rate / (2 K).
 *   A(z) = (a + z^-K) / (1 + a z^-K), a = dispersion; C = A^M, M = sections (M = 0: C = 1).
 *   P(z) = (1 - c) / (1 - c z^-1), c = damping.
 *   L = round(T rate) - round(M K (1 - a) / (1 + a)): the period less the cascade's delay at 0 Hz; L < 1 is refused.
 *   g = -10^(-3 T / t60_s) (reflections invert); t60_s = 0: g = 0, a single pass.  |g| above 0.9999 is refused.
 *   U = C P z^-L, H_low = U / (1 - g U).
 *   B(z): a Butterworth low-pass of even order lowpass_order at f_t, outside the loop, as order / 2 biquads.  With
 *   W = tan(pi / (2 K)) and, for section i < order / 2, q = 2 sin(pi (2 i + 1) / (2 order)) W:  a0 = (1 + q) + W W,
 *   b0 = b2 = (W W) / a0, b1 = 2 b0, a1 = (2 (W W - 1)) / a0, a2 = ((1 - q) + W W) / a0;
 *   section(z) = (b0 + b1 z^-1 + b2 z^-2) / (1 + a1 z^-1 + a2 z^-2).  Order 0, or K = 1, leaves B out.
 * High chirps (off when high_gain = 0, and then not evaluated).  A_h(z) = (a_h + z^-1) / (1 + a_h z^-1), a_h =
 *   high_dispersion; L_h = max(1, round(high_delay T rate)); g_h from high_t60_s as g from t60_s;
 *   U_h = A_h^M_h z^-L_h, M_h = high_sections; H_high = U_h / (1 - g_h U_h).
 * Sum.  H_c(z) = gain / sqrt(S) sum over s ascending of (B H_low + high_gain H_high), c = L, R.  |U| <= 1 on and outside the
 *   unit circle and |g| < 1: no denominator comes near 0.
 * Powers.  A^M and A_h^M_h by square-and-multiply on the complex value from M's highest bit down: r = A; for every lower bit
 *   r = r r, and r = r A when the bit is set.
 * Frames.  E = last ? min(last, F) : F.  N = 2^log2_points when set, else the smallest power of two >= max(1024, 2 E);
 *   E > N / 2 and N > 2^22 are refused.  R = MC_SPRING_RADIUS = 1e8, rho = R^(1/N).  For bin k: z_k^-1 = rho^-1
 *   e^(-2 pi i k / N) (z^-q has the magnitude exp(-q ln(R) / N) and the angle -((k q) mod N) / N turns, reduced in integers),
 *   X[k] = H_L(z_k) + i H_R(z_k), x = the inverse N-point transform of X, and for t < E
 *     y_L[t] = Re x[t] rho^t,  y_R[t] = Im x[t] rho^t.
 *   By construction y[t] = sum over m >= 0 of h[t + m N] R^-m, where h is the recursion's own impulse response: the endless
 *   tail that a transform of N points wraps around comes back R times weaker per wrap.  With |h| <= 1 per echo, what remains
 *   is at most max |g|^floor((N - E) / (L + M K (1 + a) / (1 - a))) / R of the first echo (the loop's longest round trip in
 *   the divisor): mc_ir_spring_plan reports it.  rho^t = exp(t ln(R) / N) <= 1e4 for t < N / 2.
 * Store.  llrint(y 2^40) (to nearest, ties to even) into the 64-bit accumulator of mc_ir_room's rule, written once per frame
 *   and channel: no atomics and no sums in arrival order.  Frame = (float)(late + direct + reflections + acc 2^-40).  Frame
 *   t is a function of (struct, rate, N, t) alone: the same struct stores the same bits in any slot on any run, and with
 *   log2_points set so do loads of different F on the frames both have.
 *   |y| < 2^23, so the rounded value fits: gain <= 16, sqrt(3) for three springs, echoes of at most 1 each that all overlap
 *   sum to 1 / (1 - 0.9999), the low-pass's taps sum to about 2 in magnitude and high_gain <= 16: 16 sqrt(3) (2 + 16) 1e4 = 5e6. */
#define MC_SPRING_MAX 3             /* springs */
#define MC_SPRING_MAX_STRETCH 64    /* K */
#define MC_SPRING_RADIUS 1e8        /* R */
#define MC_SPRING_MAX_LOG2 22       /* N <= 2^22, E <= 2^21 */
typedef struct {
    uint32_t struct_size;     /* sizeof(mc_ir_spring) = 80 */
    uint32_t sections;        /* M: 0 .. 512 */
    float transition_hz;      /* finite, (0, rate / 2] */
    float dispersion;         /* a: [0, 0.95] */
    float delay_ms[3];        /* finite, 0 (absent) or (0, 10000]; the present springs first, at least one */
    float t60_s;              /* 0 (one pass) or finite in [0.001, 1000] */
    float damping;            /* c: [0, 0.95] */
    uint32_t lowpass_order;   /* 0, or even 2 .. 12 */
    float high_gain;          /* [0, 16]; 0 = no high chirps */
    uint32_t high_sections;   /* M_h: 0 .. 1024 */
    float high_dispersion;    /* a_h: [-0.95, 0] */
    float high_delay;         /* (0, 1]: the high loop's delay as a part of the period */
    float high_t60_s;         /* as t60_s */
    float stereo;             /* [0, 0.25]: channel R's periods are (1 + stereo) times channel L's */
    float gain;               /* finite, (0, 16] */
    uint32_t log2_points;     /* 0 = by E, or 10 .. 22 */
    uint64_t last;            /* E = last ? min(last, F) : F: frames at and after E get nothing from the spring */
} mc_ir_spring;
/* 100 sections, transition 4300 Hz, a 0.62, springs of 66 and 82 ms, t60 2.5 s, damping 0.2, low-pass order 8, high chirps at
 * 0.1 with 200 sections, a_h -0.6, half the period, 1 s; stereo 0.03, gain 1, log2_points 0, last 0 */
void mc_default_ir_spring(mc_ir_spring *s);
/* mc_synth_ir_room(..., room = NULL, ...) with the spring's term added to the generated frames; with spring NULL it is that
 * call bit for bit.  A spring together with a room or a plate is not offered.  Checked in this order, all before the engine or
 * the device is touched (MC_ERR_ARG, the message names the field, the engine stays as it was): synth as by mc_synth_ir; the
 * spring field by field in the struct's order; then synth->rate, which must be set ("the spring needs the session's rate");
 * then transition_hz against rate / 2, K, L per spring and channel ("delay_ms[s] is shorter than the dispersion's own
 * delay"), |g|, and E against N (the message says to set last); tail as by mc_load_ir_tail, with F' after F; damp, eq and
 * shape, then e, idx and nframes as by mc_synth_ir_room. */
int mc_synth_ir_spring(mc_engine *e, uint64_t idx, uint64_t nframes, const mc_ir_synth *synth, const mc_ir_spring *spring,
                       const mc_ir_shape *shape, const mc_ir_eq *eq, const mc_ir_damp *damp, const mc_ir_tail *tail);
/* What a load of `frames` frames at `rate` would do with `spring`: out = {N, K, f_t (Hz), S, M, 1 when B is in, E, the alias
 * bound in dB (20 log10 of the bound under Frames, over the low loops and, when on, the high ones; -400 when it is 0); then
 * at 8 + 2 s + c the delay L and at 14 + 2 s + c the loop gain g of spring s < 3 in channel c (0 for an absent spring);
 * 20 .. 23 are 0}.  The spring is checked as by mc_synth_ir_spring, with rate in [8000, 384000] and frames in [1, 2^24].
 * Host arithmetic only: no engine and no HIP call. */
int mc_ir_spring_plan(const mc_ir_spring *spring, uint32_t rate, uint64_t frames, double out[24]);
/* out_re_im[4 i .. 4 i + 3] = Re H_L, Im H_L, Re H_R, Im H_R at z = e^(2 pi i hz[i] / rate), on the unit circle, by the
 * functions that make the kernel's constants and in the kernel's order of operations.  The spring is checked as by
 * mc_ir_spring_plan (no frames are involved).  Host arithmetic only. */
int mc_ir_spring_response(const mc_ir_spring *spring, uint32_t rate, const double *hz, uint32_t n, double *out_re_im);
/* The plan's twenty-four numbers of the IR's last load; MC_ERR_STATE unless that load had a spring */
int mc_ir_spring_info(const mc_engine *e, uint64_t idx, double out[24]);

int mc_num_irs(const mc_engine *e);
/* out[0..3] = sum h_L, sum h_R, sum h_L(-1)^m, sum h_R(-1)^m of the truncated IR; out[4] = taps, out[5] = partitions */
int mc_ir_info(const mc_engine *e, uint64_t idx, double out[6]);

int mc_set_params(mc_engine *e, int half, const mc_cc_value *v);
int mc_get_params(const mc_engine *e, int half, mc_cc_value *v);
/* handleCC (conv.cu:255-276): ccmap = controller numbers {select,predelay,dry,wet,speed,panDry,panWet,level} */
int mc_handle_cc(mc_engine *e, int half, const uint8_t ccmap[8], uint8_t controller, int value);

/* One JACK period: host buffers in, host buffers out, returns when the output
 * is in outL/outR (like onProcess, which blocks on the GPU; conv.cu:455). */
int mc_process(mc_engine *e, const float *in1, const float *in2, float *outL, float *outR, uint64_t nframes);
/* nblocks consecutive periods, host buffers of nblocks*256 floats: the reference's per-block copies between JACK's
 * host buffers and the device (conv.cu:321-328, 431-437) for a whole run of blocks.  Any nblocks >= 1 (a multiple of
 * period/256); long runs are cut into chunks inside (parameters are sampled per chunk).  Pageable buffers (what JACK
 * hands the reference) go through the engine's pinned staging buffer, one chunk at a time.  Buffers in pinned host
 * memory - mc_host_alloc, hipHostMalloc or hipHostRegister, all four of them - are read and written by the DMA engines
 * directly: copy-in, kernels and copy-out of consecutive chunks overlap on three streams (PCIe-bound).  Returns when
 * the output is complete in outL / outR. */
int mc_process_batch(mc_engine *e, const float *in1, const float *in2, float *outL, float *outR, uint64_t nblocks);
/* pinned host memory for mc_process_batch buffers (hipHostMalloc; no reference equivalent - JACK owns its buffers) */
void *mc_host_alloc(size_t bytes);
void mc_host_free(void *p);
/* the same with device-resident buffers (16-byte aligned, as hipMalloc and block-granular slices of it are);
 * asynchronous on the engine's stream */
int mc_process_batch_device(mc_engine *e, const float *d_in1, const float *d_in2, float *d_outL, float *d_outR,
                            uint64_t nblocks);
/* Block-sliced operation - scaling batch throughput over GPUs without a data-path collective.  The output blocks
 * of a batch are independent given the input, so G engines (one per GPU) are fed the SAME batch and each finishes
 * `count` output blocks starting at block `first` of it into d_outL/d_outR (count*256 floats each).  An engine
 * transforms only the input blocks its own windows can reach (its slice, n_ref + 8192 frames before it and the
 * same distance before the next call's slice); the partition sums and inverse transforms run over the slice plus
 * the <= 33 blocks before it that the overlap-add and the predelay reach back to (count + reach-back <=
 * max_batch).  Consequences: `first` must be the same in every call, and an engine that has been called with a
 * proper slice accepts only sliced calls, no predelay change and at most three IRs cross-fading per half until
 * mc_reset (MC_ERR_STATE otherwise).
 * first = 0, count = nblocks is mc_process_batch_device. */
int mc_process_batch_slice_device(mc_engine *e, const float *d_in1, const float *d_in2, float *d_outL, float *d_outR,
                                  uint64_t nblocks, uint64_t first, uint64_t count);
/* Sharded operation: d_partial receives this engine's share of the wet signal,
 * 2*nblocks*256 floats ([L | R], overlap-added and already shifted by the predelay);
 * after the caller has summed the partials of all shards (RCCL reduce / all-reduce),
 * mc_finish_batch_device applies Q1/Q2 terms, Q8, clamp and dry mix.  Every shard must
 * see the same input and parameters.  A predelay change, or a select that makes a fourth
 * IR cross-fade in one half, re-renders the engine's history and must not arrive while a
 * batch is between its partial and its finish (MC_ERR_STATE).
 * Up to two batches may be between their partial and their finish (finishes
 * retire batches in order), so the reduce of batch k can overlap the MAC of
 * batch k+1.  A rank that does not need the output (non-root of a reduce)
 * passes NULL for d_wet_sum, d_outL and d_outR: the batch is retired and only its Q1/Q2 prefix sums are
 * recorded (two small launches; d_in1 / d_in2 may be NULL too - the sums come from the partial's front half).
 * Every shard therefore keeps the whole Q1/Q2 history, and an engine may mix the finishes from batch to batch:
 * without output, with output, or a run of blocks (mc_finish_batch_slice_device). */
int mc_partial_batch_device(mc_engine *e, const float *d_in1, const float *d_in2, float *d_partial, uint64_t nblocks);
int mc_finish_batch_device(mc_engine *e, const float *d_in1, const float *d_in2, const float *d_wet_sum,
                           float *d_outL, float *d_outR, uint64_t nblocks);
/* The finish after a REDUCE-SCATTER instead of a reduce: every shard receives the sum of the partials for ITS run of
 * blocks [first, first + count) only - d_wet_sum_slice = [L | R], count * 256 floats each (e.g. one reduce-scatter per
 * channel over the [nblocks * 256] channel halves of the partials) - and finishes those blocks into d_outL / d_outR
 * (count * 256 floats each).  d_in1 / d_in2 are the whole batch's inputs, as passed to mc_partial_batch_device.  Every
 * shard then keeps the Q1/Q2 history (it transforms the whole input anyway), no rank is a root, and each link carries
 * 1/N of what a reduce to one root funnels into that root.  first and count are multiples of period/256.  Retires the
 * batch like mc_finish_batch_device, and may alternate with it from batch to batch (a driver falls back to a reduce for a
 * batch that does not split into equal runs).  No reference
 * equivalent (the reference runs on one device, gpu.cu:38-90). */
int mc_finish_batch_slice_device(mc_engine *e, const float *d_in1, const float *d_in2, const float *d_wet_sum_slice,
                                 float *d_outL, float *d_outR, uint64_t nblocks, uint64_t first, uint64_t count);

int mc_sync(mc_engine *e);
/* pipelined engines: the engine's stream waits for everything issued so far (no host synchronisation) */
int mc_fence(mc_engine *e);
/* ... for everything except the most recently issued batch (so that the consumer of batch k - 1 can be queued
 * behind batch k without stalling batch k + 1 on the post stage of k) */
int mc_fence_older(mc_engine *e);
/* hip_stream is a hipStream_t.  NULL selects the engine's own stream, which is NON-BLOCKING: it is not ordered
 * with HIP's default stream.  A caller whose buffers are produced or consumed on the default stream (PyTorch's
 * current stream unless one is set) must pass that stream explicitly - MC_STREAM_DEFAULT, HIP's hipStreamLegacy
 * handle - or order the two with mc_sync / events. */
#define MC_STREAM_DEFAULT ((void *)1)
int mc_set_stream(mc_engine *e, void *hip_stream);
void *mc_get_stream(mc_engine *e);
double mc_avg_runtime_ms(const mc_engine *e);      /* mean ms per mc_process call after 10 warm-ups */
int mc_enable_kernel_timing(mc_engine *e, int on); /* HIP events around the MAC kernel */
int mc_get_kernel_stats(mc_engine *e, mc_kernel_stats *out, int reset);
uint64_t mc_algorithmic_bytes_per_block(const mc_engine *e); /* (4 paths + 2 inputs) * P * 2048 */
uint64_t mc_blocks_processed(const mc_engine *e);
/* Batch length (blocks, <= at_most and <= max_batch) that suits the loaded IRs best.  Batches of at least 12288 blocks and
 * one segment run as overlap-save segments of 16384 - P16 blocks (P16 = partitions of the longest loaded IR rounded up
 * to 16): whole segments waste nothing.  Below that the sum over partitions is a second-level transform in chunks of
 * 8192 - P16 + 1 blocks (16384 - P16 + 1 for IRs over 2560 partitions): whole chunks minus one block (the reach-back
 * of a block slice), a multiple of 8.  at_most shorter than a chunk is returned as it is (rounded down to 8).
 * No reference equivalent (batch calls are new). */
uint64_t mc_preferred_batch(const mc_engine *e, uint64_t at_most);

/* Diagnostics (tests only): copy `bytes` from an engine-owned device buffer to host.
 * which: 0 = IR spectra of IR `idx` (float4 [256][pstride]), 1 = delay line
 * (float4 [256][ring]), 2 = MAC output (float4 [256][max_batch]), 3 = segments,
 * 4 = wet ring, 5 = Q1/Q2 prefix ring (double [rc][4]); host-side words, no stream access: 6 = JACK-path counters
 * {parked periods used, gave up on their own, told to give up} (3 x uint64), 7 / 8 = generation of the parameter
 * pair the last process call sampled / that was published last (uint64), 9 = batches in the Q8 regime by the form
 * their cut terms took {k_drop_fft, forward transforms, time-domain tiles} and JACK periods whose cut terms came with the
 * launch before theirs (4 x uint64), 10 = batch launches by the form
 * of their partition sums {fused, split second-level transform, resident MAC} (3 x uint64), 11 = overlap-save form {batches that
 * took it, builds of its spectra} (2 x uint64), 12 / 13 / 14 = its row buffer and spectra (float4), 15 = retired (MC_ERR_ARG;
 * it reported a measurement build of the library, which no longer exists), 16 = 256-frame JACK tails by the form partition 0 took
 * {frequency domain, time domain}, counted by the kernel (2 x uint32; read behind the stream), 17 = the stored time-domain
 * taps of IR `idx` (float2 [taps], as mc_ir_info counts them; MC_ERR_STATE in the single-transform form, which keeps none).
 * fp16 storage (precision = 1; MC_ERR_STATE on an fp32 engine): 18 = the fp16 copy of IR `idx`'s spectra, four halves
 * {L.re, L.im, R.re, R.im} per entry, each the fp32 entry of item 0 times item 20, rounded to nearest even (uint2 [256][pstride]),
 * 19 = the fp16 mirror of the delay line, item 1 times 16 (uint2 [256][ring]), 20 = the power-of-two scale of IR `idx`'s copy
 * (one float).  Either precision: 21 = the gains of the delay line's slots, {L<-in1, L<-in2, R<-in1, R<-in2} per voice row
 * (float4 [3][ring]).  Items 1, 18, 19, 20 and 21 leave the JACK path and wait for the stream, as every device buffer here does.
 * Items 0, 18 and 20 also take the merged-IR entries, idx = 256 .. 259 ([half][buffer]: what a half's IRs were summed into when
 * more of them were cross-fading than there are voices); an entry that was never allocated answers MC_ERR_ARG, as an
 * unloaded IR does.  dims[0..3] receive {pstride, ring, max_batch, wet ring length} when non-null. */
int mc_debug_read(mc_engine *e, int which, uint64_t idx, void *dst, uint64_t offset_bytes, uint64_t bytes,
                  uint64_t dims[4]);

#ifdef __cplusplus
}
#endif
#endif
