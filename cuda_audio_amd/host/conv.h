// conv.h — the reference's `Convolution` class surface (src/conv.h:30-86) as a
// thin C++ front of the MI355X engine: same base classes, same public members
// (cc[2] with the CC struct, capture/playback ports, onProcess, onStart,
// avgRuntime, prepare, onMidiMessage), same macros.  All arithmetic happens in
// libmcconv.so through the C ABI of include/mcconv.h; there are no device
// buffers or kernels on this side.
#pragma once
#include <cstddef>
#include <cstdint>
#include <optional>
#include <string>
#include <vector>

#include "../../include/mcconv.h"
#include "gpu.h"
#include "jackclient.h"
#include "midi.h"
#include "wav.h"

#ifndef CONV_DEFAULT_FFTSIZE
#define CONV_DEFAULT_FFTSIZE (512 * 256)
#endif
#ifndef CONV_MAX_SPEED
#define CONV_MAX_SPEED 1024
#endif
#ifndef CONV_MAX_PREDELAY
#define CONV_MAX_PREDELAY 8192
#endif
// CONV_GRIDSIZE / CONV_BLOCKSIZE (conv.h:14-20) configured the reference's
// grid-stride launches; launch shapes are internal to the engine here.

struct mc_group;

class Convolution : public JackClient, public RawMidi::MessageHandler {
public:
    struct CC {
        RawMidi::Device* device = nullptr;
        uint8_t message = 0;
        uint8_t select = 0, predelay = 0, dry = 0, wet = 0, speed = 0, panDry = 0, panWet = 0, level = 0;
        struct {
            size_t select = 0;    // [0, number of IRs)
            size_t predelay = 0;  // [0, 8192]
            size_t speed = 100;   // [0, 1024]
            size_t vsteps = 0;
            float dry = 0.5f;     // [0, 1]
            float wet = 0.5f;     // [0, 1]
            float panDry = 0.0f;  // [-1, 1]
            float panWet = 0.0f;  // [-1, 1]
            float level = 1.0f;   // [0, 1]
        } value;
    } cc[2];

    Convolution(const std::string& name = "Conv", size_t fftSize = CONV_DEFAULT_FFTSIZE);
    // More than one device (no reference equivalent: gpu.cu:38-90 selects one): the IR partitions are sharded over `devices`
    // and the partial wet blocks summed over RCCL (include/mcconv_group.h; needs libmcconv_rccl.so linked in).  Offline
    // rendering (processBatch) only: a JACK period does not wait for a collective.  One device = the constructor above.
    Convolution(const std::string& name, size_t fftSize, const std::vector<int>& devices, size_t maxBatch = 4096);
    ~Convolution();

    JackPort capture[2];
    JackPort playback[2];

    void onProcess(size_t nframes) override;
    void onStart() override;
    double avgRuntime() const;

    void prepare(size_t idx, const WavFile& wav, size_t nframes = 1024);
    // Convert every IR prepared from now on to the JACK client's sample rate (no reference equivalent: the reference plays
    // IR frames at whatever rate jackd runs).  The rate is known only once the client is open, so prepare() keeps the
    // decoded frames and their rate and onStart() loads them before activate().  A WAV at the client's rate (or of unknown
    // rate) is loaded as it is.  Single device only: with several devices this reports an error and exits.
    void setMatchIrRate(bool on);
    // What every IR prepared from now on goes through before it is truncated and transformed (mc_ir_shape of
    // include/mcconv.h, field for field; no reference equivalent).  Lengths and positions are frames at the rate the IR is
    // loaded at: the client's with setMatchIrRate, the WAV's own without.  The defaults switch everything off.
    struct IrShape {
        uint64_t start = 0;      // frames skipped unconditionally at the front
        float trimDb = 0.0f;     // [-120, 0]; < 0: the onset is the first frame within trimDb of the peak
        uint32_t preRoll = 0;    // frames kept before the onset
        uint64_t length = 0;     // frames kept from there; 0 = all
        bool reverse = false;
        uint64_t decayT60 = 0;   // 0 = off; else a further 60 dB of exponential decay at tap decayT60
        uint64_t fadeOut = 0;    // raised-cosine fade over the last fadeOut stored taps
        enum Normalize { None = 0, Peak = 1, Energy = 2 } normalize = None;
        float target = 1.0f;     // Peak: max |tap|; Energy: sqrt(sum (hL^2 + hR^2) / 2)
        bool off() const { return !start && trimDb == 0.0f && !length && !reverse && !decayT60 && !fadeOut && normalize == None; }
    };
    // One log line per shaped IR (onset, first kept frame, stored taps, gain).  Single device only: with several devices
    // a shape with anything on reports an error and exits.
    void setIrShape(const IrShape& shape);
    // The EQ every IR prepared from now on is filtered with on load, after its shape and before the normalisation (mc_ir_eq of
    // include/mcconv.h; no reference equivalent): up to 8 bands in order.  The bands need the client's sample rate, so
    // prepare() keeps the frames and onStart() loads them, as with setMatchIrRate; without it the frames count as being at the
    // client's rate.  One more log line per IR (bands, gain at 1 kHz).  Single device only, as setIrShape.
    struct IrEq {
        struct Band {
            enum Kind { Off = 0, LowCut, HighCut, LowShelf, HighShelf, Peak } kind = Off;
            float hz = 1000.0f, gainDb = 0.0f, q = 0.70710678f;
        };
        std::vector<Band> bands;
        bool off() const {
            for (const Band& b : bands)
                if (b.kind != Band::Off) return false;
            return true;
        }
    };
    void setIrEq(const IrEq& eq);
    // The damping every IR prepared from now on gets on load, after its shape's fade and before the EQ (mc_ir_damp of
    // include/mcconv.h; no reference equivalent): 1 to 3 crossover frequencies, ascending, and one further decay per band, low to
    // high, in seconds (0 = that band is left alone), counted from stored tap `origin`.  The seconds become frames at the
    // client's sample rate (dampFrames), so prepare() keeps the frames and onStart() loads them, as with setIrEq.  One more log
    // line per IR.  Single device only, as setIrShape.
    struct IrDamp {
        std::vector<float> xovers;
        std::vector<double> decaySeconds;  // xovers.size() + 1 of them
        uint64_t origin = 0;
        bool off() const { return xovers.empty(); }
    };
    void setIrDamp(const IrDamp& damp);
    // mc_ir_damp.decay_t60 of a decay given in seconds at rate Hz: the nearest frame, at least 1 for anything above 0
    static uint64_t dampFrames(double seconds, double rate);
    // The decay of a loaded IR, measured by the engine from the taps it convolves with (mc_ir_decay of include/mcconv.h, which
    // has the definition; no reference equivalent).  rate = 0: the client's sample rate (known from onStart() on).
    struct DecayQuery {
        unsigned rate = 0;
        std::vector<float> bands;  // centre frequencies of the band-passed rows after the broadband row, at most 10
        float q = 1.41421356f;     // per section
        float onsetDb = -20.0f;    // 0: time zero is tap 0
        uint64_t end = 0;          // taps [0, end) are analysed; 0 = all
        uint32_t curvePoints = 0;
    };
    struct Decay {
        uint64_t origin = 0, taps = 0;
        std::vector<double> rows;   // [(1 + bands) * 3 * 8]: per band and channel set (L, R, LR) {E, EDT, T20, T30, C50, C80, D50, Ts}
        std::vector<double> curve;  // [(1 + bands) * 3 * curvePoints]
        enum Set { L = 0, R = 1, LR = 2 };
        enum Field { Energy = 0, Edt, T20, T30, C50, C80, D50, Ts };
        double at(size_t band, Set set, Field f) const { return rows[(band * 3 + set) * 8 + f]; }
    };
    Decay irDecay(size_t idx, const DecayQuery& query);
    // The IrShape::decayT60 (frames) that takes a decay time of measured seconds to target seconds at rate Hz: the envelope
    // 10^(-3 m / d) adds 60 rate / d dB/s to the slope.  0 unless 0 < target < measured, both finite (an envelope only shortens).
    static uint64_t decayForRt60(double measured, double target, double rate);
    // One log line per IR loaded from now on (origin, EDT, T20, T30, C50, C80, Ts of the broadband LR row) and one more per
    // centre frequency of `bands`.  The times need the client's sample rate: prepare() keeps the frames and onStart() loads
    // them, as with setMatchIrRate.  Single device only, as setIrShape.
    void setIrDecayReport(bool on, const std::vector<float>& bands = {});
    // Aim every IR loaded from now on at a decay time of `seconds` (0 = off): it is loaded, its broadband LR T30 (T20 when the
    // curve does not reach -35 dB) is measured, and when the target is shorter it is loaded again with the decayT60 that
    // takes it there, added as a slope to the shape's own decayT60.  Loaded by onStart(), single device only, as above.
    void setIrRt60(double seconds);
    // An IR the engine generates from a seed instead of decoding a WAV (mc_ir_synth of include/mcconv.h; no reference
    // equivalent): times in seconds, turned into frames at the client's sample rate by rint, as setIrDamp's are, so prepareSynth()
    // keeps the numbers and onStart() generates.  What is not given is mc_default_ir_synth's.  The shape, EQ, damping, decay report
    // and rt60 aim that are set apply to it as to a WAV.  Two log lines per IR: frames, seed and reflections kept, then the
    // shaped load's.  Single device only, as setIrShape.
    struct IrSynth {
        double lengthSeconds = 1.0, t60Seconds = 0.0;  // frames, t60
        uint64_t seed = 0;
        double startSeconds = 0.0, buildUpSeconds = 0.0;  // late_start, build_up
        float late = 1.0f, direct = 0.0f;                 // late_gain, direct
        uint32_t early = 0;                               // n_early
        double earlyFirstSeconds = 0.0, earlyLastSeconds = 0.0;
        float earlyGain = 1.0f, width = 1.0f;
    };
    void prepareSynth(size_t idx, const IrSynth& synth, size_t nframes = 1024);
    // The same from a filled mc_ir_synth (frames at synth.rate; rate 0 only without EQ and damping), generated at once.
    void prepareSynth(size_t idx, const mc_ir_synth& synth, size_t nframes = 1024);
    // A line of an IR index that starts with "synth:" - synth:LENGTH_S:T60_S[:key=value,...] - as an IrSynth; irargs.cpp has the
    // grammar and the keys.  False, with the reason in `why`, for a malformed line.
    static bool parseSynth(const std::string& line, IrSynth& out, std::string& why);
    // mc_ir_synth of an IrSynth at rate Hz
    static mc_ir_synth synthFrames(const IrSynth& synth, double rate);

    // A rectangular room whose reflections the engine renders (mc_ir_room and mc_synth_ir_room of include/mcconv.h, the
    // image-source method; no reference equivalent): metres, and seconds turned into frames at the client's sample rate by rint,
    // so prepareRoom() keeps the numbers and onStart() renders.  `late` is an optional late field and reflections of IrSynth's
    // under the room's (its length is the IR's; late and direct default to 0, because the room supplies the direct sound).
    // What is not given is mc_default_ir_room's.  The shape, EQ, damping, reports and rt60 aim that are set apply as to a WAV,
    // and so does the tail step: the floor is measured on the room alone, then the IR is rendered again with the tail, which
    // lets a short rendering run out at its own slope.  One more log line per IR: order, images kept, the direct sound's delay.
    // Single device only, as setIrShape.
    // Directional microphones and a directional source (mc_ir_room_mics and mc_synth_ir_room_mics): `directional` is set by any
    // of the line's keys mic, aim, tilt, src, srcaim and srctilt, and such a room is loaded through mc_synth_ir_room_mics, in both
    // renderings of the tail flow, with one more log line: the direct sound's factors.  Patterns are alpha of
    // g = alpha + (1 - alpha) cos, angles degrees (azimuth from +x towards +y, tilt towards +z), left then right.
    // Walls and air per frequency band (mc_ir_room_bands and mc_synth_ir_room_bands): `banded` is set by any of the line's keys
    // xover, betas and air, and such a room is loaded through mc_synth_ir_room_bands, in both renderings of the tail flow, with one
    // more log line: Sabine's and Eyring's reverberation times per band.  xover cuts nXovers + 1 bands; betas gives every band one
    // value for its six walls (without it every band has `beta`), air one loss in dB per metre for every band or one per band.
    // A binaural listener (mc_ir_room_head and mc_synth_ir_room_head): `headed` is set by any of the line's keys head (the azimuth
    // the listener faces, degrees), headradius (metres), ears (their angle from the facing direction, degrees) and shadow (the
    // depth of the head-shadow shelf, [0, 1]), and such a room is loaded through mc_synth_ir_room_head, in both renderings of the
    // tail flow, with one more log line: the ears' delays, their difference and their shadow factors.  A rigid sphere at
    // `receiver` takes the receiver pair's place (spacing and axis are not used): a far-field model of an upright head, without
    // pinna, torso or elevation cues.
    struct IrRoom {
        float size[3] = {5.0f, 4.0f, 3.0f}, source[3] = {1.0f, 1.5f, 1.2f}, receiver[3] = {3.5f, 2.0f, 1.5f};
        float beta[6] = {0.9f, 0.9f, 0.9f, 0.9f, 0.9f, 0.9f};
        float spacing = 0.2f;
        uint32_t axis = 0;
        float speed = 343.0f, gain = 1.0f;
        uint32_t order = 0;
        double lastSeconds = 0.0;
        bool directional = false;
        float micPattern[2] = {1.0f, 1.0f}, micAim[2] = {0.0f, 0.0f}, micTilt[2] = {0.0f, 0.0f};
        float sourcePattern = 1.0f, sourceAim = 0.0f, sourceTilt = 0.0f;
        bool banded = false;
        uint32_t nXovers = 0, nBetas = 0, nAir = 0;  // values given by xover, betas and air
        float xovers[MC_DAMP_MAX_XOVERS] = {0.0f, 0.0f, 0.0f};
        float betas[MC_DAMP_MAX_XOVERS + 1] = {0.9f, 0.9f, 0.9f, 0.9f}, air[MC_DAMP_MAX_XOVERS + 1] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool headed = false;
        float headFacing = 0.0f, headRadius = 0.0875f, headEars = 90.0f, headShadow = 1.0f;
        IrSynth late;
        IrRoom() { late.late = 0.0f; }
    };
    void prepareRoom(size_t idx, const IrRoom& room, size_t nframes = 1024);
    // A line of an IR index that starts with "room:" - room:LENGTH_S:LX,LY,LZ:SX,SY,SZ:RX,RY,RZ[:key=value,...], with t60 and
    // parseSynth's keys for the late field - as an IrRoom; irargs.cpp has the grammar and the keys.  False, with the reason in
    // `why`, for a malformed line.
    static bool parseRoom(const std::string& line, IrRoom& out, std::string& why);
    // mc_ir_room of an IrRoom at rate Hz
    static mc_ir_room roomFrames(const IrRoom& room, double rate);
    // mc_ir_room_mics of a directional IrRoom
    static mc_ir_room_mics roomMics(const IrRoom& room);
    // mc_ir_room_bands of a banded IrRoom
    static mc_ir_room_bands roomBands(const IrRoom& room);
    // mc_ir_room_head of a headed IrRoom
    static mc_ir_room_head roomHead(const IrRoom& room);

    // A plate reverberator whose modes the engine sums (mc_ir_plate and mc_synth_ir_plate of include/mcconv.h; no reference
    // equivalent): metres, millimetres, Hz and seconds, the length and `last` turned into frames at the client's sample rate by
    // rint, so preparePlate() keeps the numbers and onStart() generates.  What is not given is mc_default_ir_plate's.  The shape,
    // EQ, damping, tail, reports and rt60 aim that are set apply as to a WAV.  One more log line per IR: the modes kept, those
    // that sound per channel, their range and the stiffness.  Single device only, as setIrShape.
    struct IrPlate {
        double lengthSeconds = 1.0;
        float size[2] = {2.04f, 0.97f};
        float thickness = 0.5f;                         // mm
        float material[3] = {200.0f, 7850.0f, 0.3f};    // GPa, kg/m^3, Poisson's ratio: steel
        float driver[2] = {0.83f, 0.41f};
        float pickup[2][2] = {{0.31f, 0.67f}, {1.57f, 0.29f}};
        float low = 20.0f, high = 0.0f;
        float t60[2] = {4.0f, 1.0f};
        float damp = 10000.0f, gain = 1.0f;
        double lastSeconds = 0.0;
    };
    void preparePlate(size_t idx, const IrPlate& plate, size_t nframes = 1024);
    // A line of an IR index that starts with "plate:" - plate:LENGTH_S[:key=value,...] - as an IrPlate; irargs.cpp has the grammar
    // and the keys.  False, with the reason in `why`, for a malformed line.
    static bool parsePlate(const std::string& line, IrPlate& out, std::string& why);
    // mc_ir_plate of an IrPlate at rate Hz
    static mc_ir_plate plateFrames(const IrPlate& plate, double rate);

    // A spring reverberation tank whose response the engine evaluates bin by bin (mc_ir_spring and mc_synth_ir_spring of
    // include/mcconv.h; no reference equivalent): Hz, milliseconds and seconds, the length and `last` turned into frames at the
    // client's sample rate by rint, so prepareSpring() keeps the numbers and onStart() generates.  What is not given is
    // mc_default_ir_spring's.  The shape, EQ, damping, tail, reports and rt60 aim that are set apply as to a WAV.  One more log
    // line per IR: the transform's size, the stretch and the transition, the springs' delays and the alias bound.  Single device
    // only, as setIrShape.
    struct IrSpring {
        double lengthSeconds = 1.0;
        unsigned sections = 100;
        float transition = 4300.0f, dispersion = 0.62f;
        float delayMs[3] = {66.0f, 82.0f, 0.0f};
        float t60 = 2.5f, damping = 0.2f;
        unsigned lowpass = 8;
        float high = 0.1f;
        unsigned highSections = 200;
        float highDispersion = -0.6f, highDelay = 0.5f, highT60 = 1.0f;
        float stereo = 0.03f, gain = 1.0f;
        unsigned points = 0;  // log2 of the transform's size, 0 = by the length
        double lastSeconds = 0.0;
    };
    void prepareSpring(size_t idx, const IrSpring& spring, size_t nframes = 1024);
    // A line of an IR index that starts with "spring:" - spring:LENGTH_S[:key=value,...] - as an IrSpring; irargs.cpp has the
    // grammar and the keys.  False, with the reason in `why`, for a malformed line.
    static bool parseSpring(const std::string& line, IrSpring& out, std::string& why);
    // mc_ir_spring of an IrSpring at rate Hz
    static mc_ir_spring springFrames(const IrSpring& spring, double rate);

    // An IR the engine deconvolves from the recording of an exponential sine sweep played through a room (mc_sweep and
    // mc_load_ir_sweep of include/mcconv.h; no reference equivalent): times in seconds, turned into frames at the client's
    // sample rate by rint, so prepareSweep() keeps the numbers and the recording and onStart() deconvolves.  The recording
    // must be at the client's rate (it is not converted).  irLengthSeconds 0: what the recording holds past the sweep.  The
    // shape, EQ, damping, decay report and rt60 aim that are set apply to it as to a WAV.  Two log lines per IR: the sweep's,
    // the recording's and the IR's frames and the offset, then the shaped load's.  Single device only, as setIrShape.
    struct IrSweep {
        std::string recording;  // path of the recording (index lines); file to write (--write-sweep)
        double lengthSeconds = 1.0;
        float f1 = 20.0f, f2 = 20000.0f, amp = 0.5f;
        double fadeInSeconds = 0.0, fadeOutSeconds = 0.0;
        double offsetSeconds = 0.0;    // may be negative: keeps pre-roll
        double irLengthSeconds = 0.0;
    };
    void prepareSweep(size_t idx, const IrSweep& sweep, const WavFile& recording, size_t nframes = 1024);
    // A line of an IR index that starts with "sweep:" - sweep:RECORDING.wav:LENGTH_S:F1:F2[:key=value,...] - as an IrSweep;
    // irargs.cpp has the grammar and the keys.  False, with the reason in `why`, for a malformed line.
    static bool parseSweep(const std::string& line, IrSweep& out, std::string& why);
    // mc_sweep of an IrSweep at rate Hz
    static mc_sweep sweepFrames(const IrSweep& sweep, double rate);
    // The sweep at rate Hz in both channels of a 24-bit WAV file at sweep.recording (mc_sweep_generate, WavFile::write).
    // False, with the reason in `why`, when the engine has no sweep, refuses it, or the file cannot be written.
    static bool writeSweep(const IrSweep& sweep, unsigned rate, std::string& why);

    // The noise floor of a loaded IR, searched for by the engine in the taps it convolves with (mc_ir_floor of include/mcconv.h,
    // which has the method; no reference equivalent): the broadband row group and, with 1 to 3 crossovers, one per band of
    // IrDamp's split.  Everything else of the query is mc_default_floor_query's.  rate = 0: the client's sample rate.
    struct Floor {
        uint64_t origin = 0, taps = 0;
        mc_floor_query query;
        std::vector<double> rows;  // [groups * 3 * 8]: per group and channel set {E, Nz, knee, T, peak to noise dB, w, last change, status}
        enum Field { Energy = 0, Noise, Knee, T, PeakToNoise, Interval, LastChange, Status };
        size_t groups() const { return rows.size() / 24; }
        double at(size_t group, Decay::Set set, Field f) const { return rows[(group * 3 + set) * 8 + f]; }
    };
    Floor irFloor(size_t idx, const std::vector<float>& xovers = {}, unsigned rate = 0);
    // One log line per IR loaded from now on and row group (knee, late decay time, noise level, peak to noise, interval and
    // status of the LR row), over the bands of setIrFloorXovers.  Loaded by onStart(), single device only, as setIrDecayReport.
    void setIrFloorReport(bool on);
    // The crossovers of the floor report's bands and of the tail step's (at most 3, ascending)
    void setIrFloorXovers(const std::vector<float>& xovers);
    // The echo density of a loaded IR and the mixing time it gives, measured by the engine from the taps it convolves with
    // (mc_ir_density of include/mcconv.h, which has the definition; no reference equivalent).  Seconds become taps at the client's
    // rate: the window spans 2 H + 1 taps with H = floor(windowSeconds rate / 2 + 0.5), the hop is rint(hopSeconds rate), at least
    // 1; 0 leaves either to the engine (20 ms, a quarter of H).  t60Seconds > 0 is the decay undone inside each window; autoT60
    // takes the broadband LR T30 of irDecay in its place and, where that is NaN, nothing.
    struct DensityQuery {
        double windowSeconds = 0.0, hopSeconds = 0.0, t60Seconds = 0.0;
        bool autoT60 = false;
    };
    struct Density {
        uint64_t origin = 0, taps = 0, centres = 0;
        double rows[24];  // per channel set (L, R, LR) {mixing tap, mixing time s, eta[0], max eta, its tap, mean eta after, silent windows, status}
        enum Field { Mix = 0, MixSeconds, First, Max, MaxTap, MeanAfter, Silent, Status };
        double at(Decay::Set set, Field f) const { return rows[set * 8 + f]; }
    };
    Density irDensity(size_t idx, const DensityQuery& query);
    // One log line per IR loaded from now on (origin, mixing tap and time, first, largest and later density, silent windows and
    // status of the LR row).  Loaded by onStart(), single device only, as setIrDecayReport.
    void setIrDensityReport(bool on, const DensityQuery& query);
    // The arguments of --ir-density-window and --ir-density-hop (seconds, > 0) and of --ir-density-t60 (seconds, > 0, or auto) into
    // `out`.  False, with the reason in `why`, for a malformed one.
    static bool parseDensity(const std::string& option, const std::string& arg, DensityQuery& out, std::string& why);
    // The interaural cross-correlation of a loaded IR, measured by the engine from the taps it convolves with (mc_ir_iacc of
    // include/mcconv.h, which has the definition; no reference equivalent): IACF over lags of +/- lagSeconds (1 ms unless given;
    // floor(lagSeconds rate + 0.5) taps at the client's rate) and its largest magnitude, over the early (80 ms), the late and the whole
    // IR, broadband and in one row group per band.
    struct IaccQuery {
        std::vector<float> bands;
        double lagSeconds = 0.0;
        bool lagGiven = false;
    };
    struct Iacc {
        uint64_t origin = 0, taps = 0, split = 0;  // split: the first late tap
        uint32_t maxLag = 0;
        std::vector<double> rows;  // per group and window {E_L, E_R, IACC, tau* taps, IACF(tau*), IACF(0), L over R dB, status}
        enum Window { Early = 0, Late, All };
        enum Field { EnergyL = 0, EnergyR, Peak, Lag, AtLag, Iacf0, LevelDb, Status };
        double at(size_t group, Window w, Field f) const { return rows[(group * 3 + w) * 8 + f]; }
    };
    Iacc irIacc(size_t idx, const IaccQuery& query);
    // One log line per IR loaded from now on and window of the broadband group, and one per band for the whole IR (origin, IACC,
    // tau* in taps and ms, IACF(0), level difference, status).  Loaded by onStart(), single device only, as setIrDecayReport.
    void setIrIaccReport(bool on, const IaccQuery& query);
    // The argument of --ir-iacc-lag (seconds, [0, 1]) or of --ir-iacc-bands (HZ[,HZ...], at most 10) into `out`.  False, with the
    // reason in `why`, for a malformed one.
    static bool parseIacc(const std::string& option, const std::string& arg, IaccQuery& out, std::string& why);
    // The speech transmission index of a loaded IR, measured by the engine from the taps it convolves with (mc_ir_sti of
    // include/mcconv.h, which has the definition; no reference equivalent): the seven octaves 125 Hz .. 8 kHz, IEC 60268-16's 14
    // modulation frequencies and its weights for male speech, at the client's rate.  snrDb: empty, or seven signal-to-noise
    // ratios in dB, one per octave, of stationary noise in the room.
    struct StiQuery {
        std::vector<float> snrDb;
    };
    struct Sti {
        uint64_t origin = 0, taps = 0;
        size_t bands = 0;
        double sti[3] = {0.0, 0.0, 0.0};  // L, R, LR
        std::vector<double> rows;         // per group (0 broadband, then the bands) and set {E, MTI, status, 0}
        enum Field { Energy = 0, Mti, Status };
        double at(size_t group, Decay::Set set, Field f) const { return rows[(group * 3 + set) * 4 + f]; }
    };
    Sti irSti(size_t idx, const StiQuery& query);
    // One log line per IR loaded from now on and channel set (origin, STI and its rating, the seven bands' MTI, status: 1 when a
    // band of the set has no energy).  Loaded by onStart(), single device only, as setIrDecayReport.
    void setIrStiReport(bool on, const StiQuery& query);
    // The argument of --ir-sti-snr (DB[,DB...]: one value for all seven octaves or seven, each in [-60, 120]) into `out`.  False,
    // with the reason in `why`, for a malformed one.
    static bool parseSti(const std::string& arg, StiQuery& out, std::string& why);
    // "bad", "poor", "fair", "good" or "excellent" at the edges 0.30, 0.45, 0.60, 0.75; "none" for NaN
    static const char* stiRating(double sti);
    // The frequency response of a loaded IR, measured by the engine from the taps it convolves with (mc_ir_response of
    // include/mcconv.h, which has the definition; no reference equivalent): the whole span from the origin, on the grid of 24
    // points per octave from 20 Hz to min(20 kHz, 0.45 rate) at the client's rate (mc_response_grid), with the power |H|^2 of each
    // channel smoothed over smoothOctaves (mc_response_smooth).
    struct ResponseQuery {
        double smoothOctaves = 1.0;
    };
    struct Response {
        uint64_t origin = 0, taps = 0;
        std::vector<float> hz;
        std::vector<double> resp;      // per channel (L, R) and frequency {Re H, Im H, group delay in taps from the origin}
        std::vector<double> smoothed;  // per channel and frequency: |H|^2, smoothed
        double rows[8] = {};           // per channel {E, A, status, 0}
        double re(int c, size_t f) const { return resp[((size_t)c * hz.size() + f) * 3]; }
        double im(int c, size_t f) const { return resp[((size_t)c * hz.size() + f) * 3 + 1]; }
        double delay(int c, size_t f) const { return resp[((size_t)c * hz.size() + f) * 3 + 2]; }
        size_t nearest(double f) const;  // the grid point nearest to f Hz, in octaves
    };
    Response irResponse(size_t idx, const ResponseQuery& query);
    // One log line per IR loaded from now on and channel (origin, the smoothed level at 1 kHz, the levels of the octaves 31.5 Hz ..
    // 16 kHz below 0.45 rate relative to it, the group delay at 1 kHz, status: 1 for a silent channel).  Loaded by onStart(),
    // single device only, as setIrDecayReport.
    void setIrResponseReport(bool on, const ResponseQuery& query);
    // The argument of --ir-response-smooth (OCTAVES in [0, 10]) into `out`.  False, with the reason in `why`, for a malformed one.
    static bool parseResponse(const std::string& arg, ResponseQuery& out, std::string& why);
    // The tail step every IR loaded from now on goes through (mc_ir_tail of include/mcconv.h; no reference equivalent): the IR
    // is loaded as it is, its floor is measured in the bands of setIrFloorXovers, and it is loaded again with every band cut at
    // its knee (Cut) or cross-faded there into decaying noise (Extend) ahead of its shape, EQ and damping.  An IR whose
    // broadband peak-to-noise ratio is under margin_db + span_db of the search (30 dB) is left as it is, with a log line that
    // says so, and so is a generated one without a room, which has no floor.  Seconds become frames at the client's rate by rint.  Loaded by
    // onStart(), single device only.  kneeAtMix (Extend only): every band the floor search placed gets its knee moved to the
    // mixing tap irDensity measures on the same load (the LR row, setIrDensityReport's query), its levels sliding along its own line
    // (mc_ir_tail_move_knee): the hand-over point of a rendered room, which has no floor to find.  A density that never reaches 1
    // leaves the floor's knees and logs a warning.  widthFromIacc (Extend only; width=iacc): the noise's width comes from the
    // late broadband IACF(0) that irIacc measures on the same load (setIrIaccReport's lag), 1 - rho clamped to [0, 1]
    // (mc_ir_tail_width_from_iacc), so that the tail is as correlated as the field it continues; a late window without a
    // correlation (status 1) leaves `width` and logs a warning.
    struct IrTail {
        enum Mode { Off = 0, Cut = 1, Extend = 2 } mode = Off;
        double fadeSeconds = 0.0;    // cross-fade that ends at each knee
        double lengthSeconds = 0.0;  // frames the step hands on; 0: as many as came in
        uint64_t seed = 0;
        float width = 1.0f;
        bool kneeAtMix = false;
        bool widthFromIacc = false;
    };
    void setIrTail(const IrTail& tail);
    // The argument of --ir-tail, cut|extend[:key=value,...], as an IrTail; irargs.cpp has the grammar and the keys.  False, with the
    // reason in `why`, for a malformed one.
    static bool parseTail(const std::string& arg, IrTail& out, std::string& why);
    // The phase step every IR loaded from now on goes through (mc_ir_phase of include/mcconv.h; no reference equivalent): the
    // frames are replaced by the minimum-phase IR of the same magnitude response, after the conversion and the tail step and
    // ahead of the shape, EQ and damping, which takes out the delay a short IR carries inside it.  One log line per load tells
    // the delay removed (frames and ms at the client's rate) and what the truncation to the IR's length kept.  Loaded by
    // onStart(), single device only.  A generated IR has no phase step and is loaded as it is, with a log line that says so.
    struct IrPhase {
        bool minimum = false;
        float floorDb = 120.0f;  // [40, 300]: how far below its largest bin the spectrum is followed
        unsigned overLog2 = 3;   // the transform is 2^overLog2 times the IR's length rounded up to a power of two; 1 .. 6
    };
    void setIrPhase(const IrPhase& phase);
    // The argument of --ir-phase, minimum[:key=value,...], as an IrPhase; irargs.cpp has the grammar and the keys.  False, with the
    // reason in `why`, for a malformed one.
    static bool parsePhase(const std::string& arg, IrPhase& out, std::string& why);
    // The filter step every IR loaded from now on goes through (mc_ir_filter of include/mcconv.h; no reference equivalent): the
    // frames are convolved with a second IR (a cabinet into a room, a correction FIR into a hall: one IR at run time), or that
    // one is divided out of them (a loop-back capture out of a measurement), after the phase step and ahead of the shape, EQ
    // and damping.  lr holds the filter's interleaved frames at `rate` Hz (0: the client's); the engine converts them to the
    // client's rate.  One log line per load tells the lengths and the level.  Loaded by onStart(), single device only.  A
    // generated IR has no filter step and is loaded as it is, with a log line that says so.
    struct IrFilter {
        bool on = false;
        bool deconvolve = false;
        unsigned channels = 0;     // 0 stereo, 1 left, 2 mid (MC_FILTER_STEREO / LEFT / MID)
        float regDb = 60.0f;       // [20, 200]: the regularisation of a deconvolution below the filter's strongest bin
        double keepSeconds = 0.0;  // the length the step hands on; 0 = all of a convolution, the IR's own of a deconvolution
        std::string path;          // as given on the command line
        unsigned rate = 0;
        std::vector<float> lr;
    };
    void setIrFilter(const IrFilter& filter);
    // The argument of --ir-filter, FILE.wav[:key=value,...], as an IrFilter without its frames; irargs.cpp has the grammar and the
    // keys.  False, with the reason in `why`, for a malformed one.
    static bool parseFilter(const std::string& arg, IrFilter& out, std::string& why);
    // The match step every IR loaded from now on goes through (mc_ir_match of include/mcconv.h; no reference equivalent): a match
    // EQ that gives the frames the smoothed spectrum of a target IR, or of a flat or tilted line, after the filter step and ahead
    // of the shape, EQ and damping.  lr holds the target's interleaved frames at `rate` Hz (0: the client's); the engine converts
    // them to the client's rate.  One log line per load tells the lengths, the curve's range and the level; with `report` one
    // line per grid point follows with the curve.  Loaded by onStart(), single device only.  A generated IR has no match step
    // and is loaded as it is, with a log line that says so.
    struct IrMatch {
        bool on = false;
        bool flat = false;          // no target: a line that tilts by tiltDb per octave
        bool linear = false;        // a linear-phase correction that delays the IR by delaySeconds; else minimum phase
        bool link = true;           // one curve from both channels; false: a curve per channel
        float amount = 1.0f;        // [0, 1] of the difference
        float boostDb = 12.0f, cutDb = 24.0f;  // [0, 60]: the curve's bounds
        double octaves = 1.0 / 3.0;            // [1/24, 2]: the smoothing
        double loHz = 20.0, hiHz = 0.0;        // the grid; hiHz 0: min(20000, half the client's rate)
        double delaySeconds = 0.0;
        float tiltDb = 0.0f;
        std::string path;           // as given on the command line, or "flat"
        unsigned rate = 0;
        std::vector<float> lr;
    };
    void setIrMatch(const IrMatch& match, bool report);
    // The argument of --ir-match, FILE.wav|flat[:key=value,...], as an IrMatch without its frames; irargs.cpp has the grammar and
    // the keys.  False, with the reason in `why`, for a malformed one.
    static bool parseMatch(const std::string& arg, IrMatch& out, std::string& why);
    // The parts step every IR loaded from now on goes through (mc_ir_parts of include/mcconv.h; no reference equivalent): the
    // direct sound, the early reflections and the late tail get a gain (or are muted), a delay, a width and a balance each, after
    // the match step and ahead of the shape, EQ and damping.  The direct part ends firstSeconds and the early part splitSeconds
    // after onsetSeconds; with splitAtMix the IR is loaded once without the step, its echo density is measured, and the onset and
    // the early part's end are the measurement's origin and mixing tap (80 ms after the origin when the density never reaches
    // 1).  One log line per load tells the boundaries, the parts' energies and what was lost.  Loaded by onStart(), single
    // device only.  A generated IR has no parts step and is loaded as it is, with a log line that says so.
    struct IrParts {
        bool on = false;
        bool mute[3] = {false, false, false}, swap[3] = {false, false, false}, invert[3] = {false, false, false};
        float gainDb[3] = {0.f, 0.f, 0.f};
        float width[3] = {1.f, 1.f, 1.f}, balance[3] = {0.f, 0.f, 0.f};
        double delaySeconds[3] = {0.0, 0.0, 0.0}, xfadeSeconds[2] = {0.0, 0.0};
        double onsetSeconds = 0.0, firstSeconds = 0.0025, splitSeconds = 0.08;
        bool splitAtMix = false;
    };
    void setIrParts(const IrParts& parts);
    // The argument of --ir-parts, key=value,..., as an IrParts; irargs.cpp has the grammar and the keys.  False, with the reason in
    // `why`, for a malformed one.
    static bool parseParts(const std::string& arg, IrParts& out, std::string& why);

    void onMidiMessage(const RawMidi::Device* sender, const uint8_t* buffer, size_t len) override;

    // offline rendering through the same engine: nblocks * 256 frames per channel
    void processBatch(const float* in1, const float* in2, float* outL, float* outR, size_t nblocks);
    size_t numIrs() const { return _nirs; }

private:
    mc_engine* _engine = nullptr;
    mc_group* _group = nullptr;  // != null: several devices; _engine is rank 0's engine (parameters are read back from it)
    size_t _fftSize;
    size_t _maxBatch = 256;
    size_t _nirs = 0;
    size_t _period = 256;
    size_t _pushedVsteps[2] = {0, 0};  // cc[i].value.vsteps as last handed to the engine (see pullVsteps)
    bool _matchIrRate = false;
    struct PendingIr {
        size_t idx = 0, nframes = 1024;
        unsigned rate = 0;
        std::vector<float> lr;  // interleaved L, R frames
        IrShape shape;          // as set when the IR was prepared
        IrEq eq;
        bool match = false;     // setMatchIrRate was on
        IrDamp damp;
        bool generated = false;  // prepareSynth: `synth` instead of lr
        IrSynth synth;
        bool swept = false;  // prepareSweep: lr is the recording of `sweep`
        IrSweep sweep;
        bool roomed = false;  // prepareRoom: generated, `room` with its late field in place of `synth`
        IrRoom room = IrRoom();
        bool plated = false;  // preparePlate: generated, `plate` and nothing of `synth` but its length
        IrPlate plate = IrPlate();
        bool sprung = false;  // prepareSpring: generated, `spring` and nothing of `synth` but its length
        IrSpring spring = IrSpring();
    };
    struct SweepLoad {  // the arguments of mc_load_ir_sweep beside the recording
        mc_sweep sweep;
        int64_t offset;
        uint64_t irFrames;
    };
    struct PartsSplit {  // measureParts: the frames of the onset and of the mixing tap
        uint64_t onset, mix;
    };
    // One load of one IR: where its frames come from and every step they go through.  loadIr() reads nothing else that describes
    // the load, so a load without some of the steps is a copy of this with those fields cleared.
    struct IrLoadRequest {
        size_t idx = 0, nframes = 1024;
        // The source, exactly one of three.  Host frames: lr, `frames` of them at irRate Hz (0: at the rate they have, not
        // converted) in a session at sessionRate Hz (0: not known).  synth: the engine generates the frames at synth->rate, with the
        // reflections of `room`, its microphones directional with `mics`, its walls and air per frequency band with `bands`.  sweep:
        // lr is the recording of a sweep, `frames` frames at sweep->sweep.rate, which the engine deconvolves.
        const float* lr = nullptr;
        uint64_t frames = 0;
        unsigned irRate = 0, sessionRate = 0;
        std::optional<mc_ir_synth> synth;
        std::optional<mc_ir_room> room;
        std::optional<mc_ir_room_mics> mics;
        std::optional<mc_ir_room_bands> bands;
        std::optional<mc_ir_room_head> head;
        std::optional<mc_ir_plate> plate;  // with synth and without room: the modes of a plate are added (mc_synth_ir_plate)
        std::optional<mc_ir_spring> spring;  // with synth and without room and plate: a spring tank's response is added (mc_synth_ir_spring)
        std::optional<SweepLoad> sweep;
        // The steps, in the order the frames go through them: tail, phase, filter, match, parts (null = off; they point at the
        // object's settings, whose second IRs are not copied), then shape, damp, eq.  A generated IR goes through the tail (with a
        // room), shape, damp and eq alone.  split: the parts' boundaries as measured, in place of the settings' seconds.
        std::optional<mc_ir_tail> tail;
        const IrPhase* phase = nullptr;
        const IrFilter* filter = nullptr;
        const IrMatch* match = nullptr;
        const IrParts* parts = nullptr;
        std::optional<PartsSplit> split;
        IrShape shape;
        IrEq eq;
        IrDamp damp;
    };
    std::vector<PendingIr> _pendingIrs;  // (rate matching) prepared, loaded by onStart()
    PendingIr& pend(size_t idx, size_t nframes);
    void loadPendingIrs();
    IrLoadRequest requestNow(size_t idx, size_t nframes, const IrShape& shape, const IrEq& eq, const IrDamp& damp) const;  // no source yet; the steps that are set
    IrLoadRequest requestFor(const PendingIr& p);  // p's source at the client's rate and every step that is set; no tail, no split
    void loadIr(const IrLoadRequest& r);
    std::optional<mc_ir_tail> measureTail(const PendingIr& p);
    std::optional<PartsSplit> measureParts(const PendingIr& p, const std::optional<mc_ir_tail>& tail);
    void aimRt60(const IrLoadRequest& loaded);
    // the host's settings as the engine's structs; seconds become frames at `session` Hz
    static mc_ir_shape shapeArg(const IrShape& shape);
    static mc_ir_eq eqArg(const IrEq& eq);
    static mc_ir_damp dampArg(const IrDamp& damp, double session);
    static mc_ir_phase phaseArg(const IrPhase& phase);
    static mc_ir_filter filterArg(const IrFilter& filter, unsigned session);
    static mc_ir_match matchArg(const IrMatch& match, unsigned session);
    static mc_ir_parts partsArg(size_t idx, const IrParts& parts, double session, const std::optional<PartsSplit>& split);
    void reportDecay(size_t idx);
    void reportFloor(size_t idx);
    void reportDensity(size_t idx);
    void reportIacc(size_t idx);
    void reportSti(size_t idx);
    bool _stiReport = false;
    StiQuery _stiQuery;
    void reportResponse(size_t idx);
    bool _responseReport = false;
    ResponseQuery _responseQuery;
    bool _iaccReport = false;
    IaccQuery _iaccQuery;
    bool _densityReport = false;
    DensityQuery _densityQuery;
    bool _floorReport = false;
    std::vector<float> _floorXovers;
    IrTail _irTail;
    IrPhase _irPhase;
    IrFilter _irFilter;
    IrMatch _irMatch;
    bool _irMatchReport = false;
    IrParts _irParts;
    bool _decayReport = false;
    std::vector<float> _decayBands;
    double _rt60 = 0.0;
    IrShape _irShape;
    IrEq _irEq;
    IrDamp _irDamp;
    void pushParams();
    void pullVsteps();
};
