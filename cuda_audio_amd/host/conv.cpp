#include "conv.h"

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>

#include "../../include/mcconv_group.h"

// the multi-device driver is optional at link time (libmcconv_rccl.so): the single-device host and the stub host do without it
extern "C" {
int mc_group_create(const mc_config*, const int32_t*, uint32_t, mc_group**) __attribute__((weak));
void mc_group_destroy(mc_group*) __attribute__((weak));
mc_engine* mc_group_engine(mc_group*, uint32_t) __attribute__((weak));
int mc_group_load_ir(mc_group*, uint64_t, const float*, uint64_t, uint64_t) __attribute__((weak));
int mc_group_set_params(mc_group*, int, const mc_cc_value*) __attribute__((weak));
int mc_group_process_batch(mc_group*, const float*, const float*, float*, float*, uint64_t) __attribute__((weak));
const char* mc_group_last_error(void) __attribute__((weak));
// (weak as well: the stub host's stand-in engine has no sample-rate conversion)
int mc_load_ir_resampled(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, uint32_t, uint32_t) __attribute__((weak));
// (and no IR shaping)
void mc_default_ir_shape(mc_ir_shape*) __attribute__((weak));
int mc_load_ir_shaped(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, uint32_t, uint32_t, const mc_ir_shape*) __attribute__((weak));
int mc_ir_shape_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
// (... and no EQ)
void mc_default_ir_eq(mc_ir_eq*) __attribute__((weak));
int mc_load_ir_eq(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, uint32_t, uint32_t, const mc_ir_shape*, const mc_ir_eq*) __attribute__((weak));
int mc_ir_eq_response(const mc_ir_eq*, uint32_t, const double*, uint32_t, double*) __attribute__((weak));
// (... and no damping)
void mc_default_ir_damp(mc_ir_damp*) __attribute__((weak));
int mc_load_ir_damped(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, uint32_t, uint32_t, const mc_ir_shape*, const mc_ir_eq*, const mc_ir_damp*)
    __attribute__((weak));
int mc_ir_damp_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
// (... and no decay measurement)
void mc_default_decay_query(mc_decay_query*) __attribute__((weak));
int mc_ir_decay(mc_engine*, uint64_t, const mc_decay_query*, double*, double*, uint64_t*) __attribute__((weak));
// (... and no synthesis)
void mc_default_ir_synth(mc_ir_synth*) __attribute__((weak));
int mc_synth_ir(mc_engine*, uint64_t, uint64_t, const mc_ir_synth*, const mc_ir_shape*, const mc_ir_eq*, const mc_ir_damp*) __attribute__((weak));
int mc_ir_synth_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
// (... and no sweep capture)
void mc_default_sweep(mc_sweep*) __attribute__((weak));
int mc_sweep_generate(const mc_sweep*, float*, uint64_t, uint64_t) __attribute__((weak));
int mc_load_ir_sweep(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, const mc_sweep*, int64_t, uint64_t, const mc_ir_shape*, const mc_ir_eq*,
                     const mc_ir_damp*) __attribute__((weak));
int mc_ir_sweep_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
// ... no floor measurement and no tail step
void mc_default_floor_query(mc_floor_query*) __attribute__((weak));
int mc_ir_floor(mc_engine*, uint64_t, const mc_floor_query*, double*, uint64_t*) __attribute__((weak));
int mc_ir_tail_from_floor(const mc_floor_query*, const double*, const uint64_t*, uint64_t, mc_ir_tail*) __attribute__((weak));
void mc_default_ir_tail(mc_ir_tail*) __attribute__((weak));
// ... no density measurement and no knee to move
void mc_default_density_query(mc_density_query*) __attribute__((weak));
int mc_ir_density(mc_engine*, uint64_t, const mc_density_query*, double*, double*, uint64_t*) __attribute__((weak));
int mc_ir_tail_move_knee(mc_ir_tail*, uint32_t, uint64_t) __attribute__((weak));
// ... no IACC measurement and no width to take from it
void mc_default_iacc_query(mc_iacc_query*) __attribute__((weak));
int mc_ir_iacc(mc_engine*, uint64_t, const mc_iacc_query*, double*, double*, uint64_t*) __attribute__((weak));
int mc_ir_tail_width_from_iacc(mc_ir_tail*, double) __attribute__((weak));
// ... no STI measurement
void mc_default_sti_query(mc_sti_query*) __attribute__((weak));
int mc_ir_sti(mc_engine*, uint64_t, const mc_sti_query*, double*, double*, double*, uint64_t*) __attribute__((weak));
// ... no response measurement (the grid and the smoothing are the engine's host arithmetic: they come and go with it)
void mc_default_response_query(mc_response_query*) __attribute__((weak));
int mc_ir_response(mc_engine*, uint64_t, const mc_response_query*, const float*, const mc_response_window*, double*, double*, uint64_t*, uint64_t*)
    __attribute__((weak));
int mc_response_grid(double, double, uint32_t, float*, uint32_t) __attribute__((weak));
int mc_response_smooth(const float*, const double*, uint32_t, double, double*) __attribute__((weak));
int mc_load_ir_tail(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, uint32_t, uint32_t, const mc_ir_shape*, const mc_ir_eq*, const mc_ir_damp*,
                    const mc_ir_tail*) __attribute__((weak));
int mc_load_ir_sweep_tail(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, const mc_sweep*, int64_t, uint64_t, const mc_ir_shape*, const mc_ir_eq*,
                          const mc_ir_damp*, const mc_ir_tail*) __attribute__((weak));
int mc_ir_tail_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
void mc_default_ir_phase(mc_ir_phase*) __attribute__((weak));
int mc_load_ir_phase(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, uint32_t, uint32_t, const mc_ir_shape*, const mc_ir_eq*, const mc_ir_damp*,
                     const mc_ir_tail*, const mc_ir_phase*) __attribute__((weak));
int mc_load_ir_sweep_phase(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, const mc_sweep*, int64_t, uint64_t, const mc_ir_shape*, const mc_ir_eq*,
                           const mc_ir_damp*, const mc_ir_tail*, const mc_ir_phase*) __attribute__((weak));
int mc_ir_phase_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
void mc_default_ir_filter(mc_ir_filter*) __attribute__((weak));
int mc_load_ir_filter(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, uint32_t, uint32_t, const mc_ir_shape*, const mc_ir_eq*, const mc_ir_damp*,
                      const mc_ir_tail*, const mc_ir_phase*, const mc_ir_filter*, const float*, uint64_t) __attribute__((weak));
int mc_load_ir_sweep_filter(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, const mc_sweep*, int64_t, uint64_t, const mc_ir_shape*, const mc_ir_eq*,
                            const mc_ir_damp*, const mc_ir_tail*, const mc_ir_phase*, const mc_ir_filter*, const float*, uint64_t) __attribute__((weak));
int mc_ir_filter_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
void mc_default_ir_match(mc_ir_match*) __attribute__((weak));
int mc_load_ir_match(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, uint32_t, uint32_t, const mc_ir_shape*, const mc_ir_eq*, const mc_ir_damp*,
                     const mc_ir_tail*, const mc_ir_phase*, const mc_ir_filter*, const float*, uint64_t, const mc_ir_match*, const float*, uint64_t)
    __attribute__((weak));
int mc_load_ir_sweep_match(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, const mc_sweep*, int64_t, uint64_t, const mc_ir_shape*, const mc_ir_eq*,
                           const mc_ir_damp*, const mc_ir_tail*, const mc_ir_phase*, const mc_ir_filter*, const float*, uint64_t, const mc_ir_match*,
                           const float*, uint64_t) __attribute__((weak));
int mc_ir_match_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
int mc_ir_match_curve(const mc_engine*, uint64_t, double*, double*, double*, uint32_t) __attribute__((weak));
void mc_default_ir_parts(mc_ir_parts*) __attribute__((weak));
int mc_load_ir_parts(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, uint32_t, uint32_t, const mc_ir_shape*, const mc_ir_eq*, const mc_ir_damp*,
                     const mc_ir_tail*, const mc_ir_phase*, const mc_ir_filter*, const float*, uint64_t, const mc_ir_match*, const float*, uint64_t,
                     const mc_ir_parts*) __attribute__((weak));
int mc_load_ir_sweep_parts(mc_engine*, uint64_t, const float*, uint64_t, uint64_t, const mc_sweep*, int64_t, uint64_t, const mc_ir_shape*, const mc_ir_eq*,
                           const mc_ir_damp*, const mc_ir_tail*, const mc_ir_phase*, const mc_ir_filter*, const float*, uint64_t, const mc_ir_match*,
                           const float*, uint64_t, const mc_ir_parts*) __attribute__((weak));
int mc_ir_parts_at(mc_ir_parts*, uint64_t, uint64_t, uint64_t) __attribute__((weak));
int mc_ir_parts_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
// ... and no room
void mc_default_ir_room(mc_ir_room*) __attribute__((weak));
int mc_synth_ir_room(mc_engine*, uint64_t, uint64_t, const mc_ir_synth*, const mc_ir_room*, const mc_ir_shape*, const mc_ir_eq*, const mc_ir_damp*,
                     const mc_ir_tail*) __attribute__((weak));
int mc_ir_room_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
// ... or a room without directional microphones
void mc_default_ir_room_mics(mc_ir_room_mics*) __attribute__((weak));
int mc_synth_ir_room_mics(mc_engine*, uint64_t, uint64_t, const mc_ir_synth*, const mc_ir_room*, const mc_ir_room_mics*, const mc_ir_shape*,
                          const mc_ir_eq*, const mc_ir_damp*, const mc_ir_tail*) __attribute__((weak));
int mc_ir_room_mics_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
// ... or a room whose walls are the same at every frequency
void mc_default_ir_room_bands(mc_ir_room_bands*) __attribute__((weak));
int mc_synth_ir_room_bands(mc_engine*, uint64_t, uint64_t, const mc_ir_synth*, const mc_ir_room*, const mc_ir_room_mics*, const mc_ir_room_bands*,
                           const mc_ir_shape*, const mc_ir_eq*, const mc_ir_damp*, const mc_ir_tail*) __attribute__((weak));
int mc_ir_room_bands_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
// ... or a room without a binaural listener
void mc_default_ir_room_head(mc_ir_room_head*) __attribute__((weak));
int mc_synth_ir_room_head(mc_engine*, uint64_t, uint64_t, const mc_ir_synth*, const mc_ir_room*, const mc_ir_room_mics*, const mc_ir_room_bands*,
                          const mc_ir_room_head*, const mc_ir_shape*, const mc_ir_eq*, const mc_ir_damp*, const mc_ir_tail*) __attribute__((weak));
int mc_ir_room_head_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
// ... or no plate
void mc_default_ir_plate(mc_ir_plate*) __attribute__((weak));
int mc_synth_ir_plate(mc_engine*, uint64_t, uint64_t, const mc_ir_synth*, const mc_ir_plate*, const mc_ir_shape*, const mc_ir_eq*, const mc_ir_damp*,
                      const mc_ir_tail*) __attribute__((weak));
int mc_ir_plate_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
// ... or no spring
void mc_default_ir_spring(mc_ir_spring*) __attribute__((weak));
int mc_synth_ir_spring(mc_engine*, uint64_t, uint64_t, const mc_ir_synth*, const mc_ir_spring*, const mc_ir_shape*, const mc_ir_eq*, const mc_ir_damp*,
                       const mc_ir_tail*) __attribute__((weak));
int mc_ir_spring_info(const mc_engine*, uint64_t, double*) __attribute__((weak));
}

namespace {
void check(int rc, const char* what) {
    // the reference asserts on every CUDA/cuFFT return code (asserts enabled): abort with a message
    if (rc != MC_OK) {
        Log::error("conv", "%s failed: %s", what, mc_last_error());
        std::abort();
    }
}
}  // namespace

Convolution::Convolution(const std::string& name, size_t fftSize)
    : JackClient(name), capture{nullptr, nullptr}, playback{nullptr, nullptr}, _fftSize(fftSize) {
    mc_config cfg;
    mc_default_config(&cfg);
    cfg.n_ref = fftSize;
    cfg.max_batch = 256;
    check(mc_create(&cfg, &_engine), "mc_create");
}

Convolution::Convolution(const std::string& name, size_t fftSize, const std::vector<int>& devices, size_t maxBatch)
    : JackClient(name), capture{nullptr, nullptr}, playback{nullptr, nullptr}, _fftSize(fftSize), _maxBatch(maxBatch) {
    mc_config cfg;
    mc_default_config(&cfg);
    cfg.n_ref = fftSize;
    cfg.max_batch = (uint32_t)maxBatch;
    if (devices.size() <= 1) {
        if (!devices.empty()) cfg.device = devices[0];
        check(mc_create(&cfg, &_engine), "mc_create");
        return;
    }
    if (!mc_group_create) {
        Log::error("conv", "%zu devices requested but the multi-device driver (libmcconv_rccl.so) is not linked in", devices.size());
        std::abort();
    }
    std::vector<int32_t> devs(devices.begin(), devices.end());
    if (mc_group_create(&cfg, devs.data(), (uint32_t)devs.size(), &_group) != MC_OK) {
        Log::error("conv", "mc_group_create failed: %s", mc_group_last_error());
        std::abort();
    }
    _engine = mc_group_engine(_group, 0);
}

Convolution::~Convolution() {
    if (_group) mc_group_destroy(_group);  // (owns its engines)
    else mc_destroy(_engine);
    _group = nullptr;
    _engine = nullptr;
}

void Convolution::onStart() {
    loadPendingIrs();  // (rate matching: the client's rate is known from here on)
    // reference conv.cu:197-204: activate first, then register 2 outputs and 2 inputs
    activate();
    playback[0] = addOutput("playback_1");
    playback[1] = addOutput("playback_2");
    capture[0] = addInput("capture_1");
    capture[1] = addInput("capture_2");
}

void Convolution::setMatchIrRate(bool on) {
    if (on && _group) {
        Log::error("conv", "IR rate matching is not available with several devices (mc_group_load_ir takes no rate)");
        std::exit(2);
    }
    _matchIrRate = on;
}

void Convolution::setIrShape(const IrShape& shape) {
    if (!shape.off() && _group) {
        Log::error("conv", "IR shaping is not available with several devices (mc_group_load_ir takes no shape)");
        std::exit(2);
    }
    _irShape = shape;
}

void Convolution::setIrEq(const IrEq& eq) {
    if (!eq.off() && _group) {
        Log::error("conv", "IR equalisation is not available with several devices (mc_group_load_ir takes no bands)");
        std::exit(2);
    }
    if (eq.bands.size() > MC_EQ_MAX_BANDS) {
        Log::error("conv", "%zu EQ bands, at most %d", eq.bands.size(), MC_EQ_MAX_BANDS);
        std::exit(2);
    }
    _irEq = eq;
}

void Convolution::setIrDamp(const IrDamp& damp) {
    if (!damp.off() && _group) {
        Log::error("conv", "IR damping is not available with several devices (mc_group_load_ir takes no damping)");
        std::exit(2);
    }
    if (damp.xovers.size() > MC_DAMP_MAX_XOVERS || (!damp.off() && damp.decaySeconds.size() != damp.xovers.size() + 1)) {
        Log::error("conv", "%zu crossovers (at most %d) need one decay per band, %zu given", damp.xovers.size(), MC_DAMP_MAX_XOVERS,
                   damp.decaySeconds.size());
        std::exit(2);
    }
    _irDamp = damp;
}

uint64_t Convolution::dampFrames(double seconds, double rate) {
    if (!(seconds > 0.0) || !std::isfinite(seconds)) return 0;
    const double f = std::nearbyint(seconds * rate);
    return f < 1.0 ? 1 : (uint64_t)f;
}

mc_ir_shape Convolution::shapeArg(const IrShape& shape) {
    mc_ir_shape s;
    mc_default_ir_shape(&s);
    s.flags = shape.reverse ? MC_SHAPE_REVERSE : 0;
    s.start = shape.start;
    s.trim_db = shape.trimDb;
    s.pre_roll = shape.preRoll;
    s.length = shape.length;
    s.decay_t60 = shape.decayT60;
    s.fade_out = shape.fadeOut;
    s.normalize = (uint32_t)shape.normalize;
    s.target = shape.target;
    return s;
}

mc_ir_eq Convolution::eqArg(const IrEq& eq) {
    mc_ir_eq q;
    mc_default_ir_eq(&q);
    for (size_t k = 0; k < eq.bands.size(); k++) q.band[k] = mc_eq_band{(uint32_t)eq.bands[k].kind, eq.bands[k].hz, eq.bands[k].gainDb, eq.bands[k].q};
    return q;
}

mc_ir_damp Convolution::dampArg(const IrDamp& damp, double session) {
    mc_ir_damp d;
    mc_default_ir_damp(&d);
    d.n_xovers = (uint32_t)damp.xovers.size();
    for (size_t k = 0; k < damp.xovers.size(); k++) d.xover_hz[k] = damp.xovers[k];
    for (size_t j = 0; j < damp.decaySeconds.size(); j++) d.decay_t60[j] = dampFrames(damp.decaySeconds[j], session);
    d.origin = damp.origin;
    return d;
}

mc_ir_phase Convolution::phaseArg(const IrPhase& phase) {
    mc_ir_phase ph;
    mc_default_ir_phase(&ph);
    ph.mode = MC_PHASE_MINIMUM;
    ph.floor_db = phase.floorDb;
    ph.over_log2 = phase.overLog2;
    return ph;
}

mc_ir_filter Convolution::filterArg(const IrFilter& filter, unsigned session) {
    mc_ir_filter fl;
    mc_default_ir_filter(&fl);
    fl.op = filter.deconvolve ? MC_FILTER_DECONVOLVE : MC_FILTER_CONVOLVE;
    fl.channels = filter.channels;
    fl.rate = filter.rate && filter.rate != session ? filter.rate : 0;
    fl.reg_db = filter.regDb;
    fl.frames_out = dampFrames(filter.keepSeconds, (double)session);
    return fl;
}

mc_ir_match Convolution::matchArg(const IrMatch& match, unsigned session) {
    mc_ir_match mt;
    mc_default_ir_match(&mt);
    mt.mode = match.flat ? MC_MATCH_FLAT : MC_MATCH_TARGET;
    mt.phase = match.linear ? MC_MATCH_LINEAR : MC_MATCH_MINIMUM;
    mt.link = match.link ? 1 : 0;
    mt.rate = !match.flat && match.rate && match.rate != session ? match.rate : 0;
    mt.lo_hz = match.loHz;
    mt.hi_hz = match.hiHz;
    mt.octaves = match.octaves;
    mt.amount = match.amount;
    mt.boost_db = match.boostDb;
    mt.cut_db = match.cutDb;
    mt.tilt_db = match.tiltDb;
    mt.delay = (uint32_t)dampFrames(match.delaySeconds, (double)session);
    return mt;
}

mc_ir_parts Convolution::partsArg(size_t idx, const IrParts& parts, double session, const std::optional<PartsSplit>& split) {
    mc_ir_parts pt;
    mc_default_ir_parts(&pt);
    pt.mode = MC_PARTS_ON;
    for (int k = 0; k < 3; k++) {
        pt.flags |= (parts.mute[k] ? MC_PARTS_MUTE(k) : 0u) | (parts.swap[k] ? MC_PARTS_SWAP(k) : 0u) | (parts.invert[k] ? MC_PARTS_INVERT(k) : 0u);
        pt.delay[k] = (int32_t)std::nearbyint(parts.delaySeconds[k] * session);
        pt.gain_db[k] = parts.gainDb[k], pt.width[k] = parts.width[k], pt.balance[k] = parts.balance[k];
    }
    for (int k = 0; k < 2; k++) pt.xfade[k] = (uint32_t)dampFrames(parts.xfadeSeconds[k], session);
    const uint64_t onset = split ? split->onset : dampFrames(parts.onsetSeconds, session);
    const uint64_t first = dampFrames(parts.firstSeconds, session);
    const uint64_t early = split ? split->mix - split->onset : dampFrames(parts.splitSeconds, session);
    if (mc_ir_parts_at(&pt, onset, std::min(first, early), early) != MC_OK) {
        Log::error("conv", "IR %zu cannot be split into parts: %s", idx, mc_last_error());
        std::exit(2);
    }
    return pt;
}

// The one way an IR reaches the engine once anything but the reference's plain load is asked of it: what the engine must have,
// the settings as its structs, the call, and the log lines of what was done.
void Convolution::loadIr(const IrLoadRequest& r) {
    const size_t idx = r.idx;
    const bool generated = r.synth.has_value();
    const bool minimum = r.phase && !generated, filtered = r.filter && !generated, matched = r.match && !generated, parted = r.parts && !generated;
    const bool tailed = r.tail.has_value(), equalised = !r.eq.off(), damped = !r.damp.off();
    if (!generated && !r.sweep && !tailed && !minimum && !filtered && !matched && !parted && !equalised && !damped && r.shape.off()) {  // (the reference's plain load)
        const bool convert = r.irRate && r.irRate != r.sessionRate;
        if (!convert) {
            check(mc_load_ir(_engine, idx, r.lr, r.frames, r.nframes), "mc_load_ir");
            return;
        }
        if (!mc_load_ir_resampled) {
            Log::error("conv", "the engine has no sample-rate conversion (mc_load_ir_resampled)");
            std::exit(2);
        }
        Log::info(name, "IR %zu: %u Hz -> %u Hz", idx, r.irRate, r.sessionRate);
        check(mc_load_ir_resampled(_engine, idx, r.lr, r.frames, r.nframes, r.irRate, r.sessionRate), "mc_load_ir_resampled");
        return;
    }

    // what the engine must have: the stub host's stand-in has mc_load_ir alone
    const struct {
        const char* dropped;  // a step that is set and that a generated IR does not go through
        bool needed, there;
        const char* lacks;
    } capabilities[] = {
        {nullptr, r.head.has_value(), mc_synth_ir_room_head && mc_default_ir_room_head && mc_ir_room_head_info, "a binaural listener in its rooms (mc_synth_ir_room_head)"},
        {nullptr, r.bands.has_value(), mc_synth_ir_room_bands && mc_default_ir_room_bands && mc_ir_room_bands_info, "frequency bands in its rooms (mc_synth_ir_room_bands)"},
        {nullptr, r.mics.has_value(), mc_synth_ir_room_mics && mc_default_ir_room_mics && mc_ir_room_mics_info, "directional microphones in its rooms (mc_synth_ir_room_mics)"},
        {nullptr, r.room.has_value(), mc_synth_ir_room && mc_default_ir_room && mc_ir_room_info, "room rendering (mc_synth_ir_room)"},
        {nullptr, r.plate.has_value(), mc_synth_ir_plate && mc_default_ir_plate && mc_ir_plate_info, "plate synthesis (mc_synth_ir_plate)"},
        {nullptr, r.spring.has_value(), mc_synth_ir_spring && mc_default_ir_spring && mc_ir_spring_info, "spring synthesis (mc_synth_ir_spring)"},
        {r.phase && generated ? "phase" : nullptr, minimum, mc_default_ir_phase && mc_load_ir_phase && mc_load_ir_sweep_phase && mc_ir_phase_info, "phase step (mc_load_ir_phase)"},
        {r.filter && generated ? "filter" : nullptr, filtered, mc_default_ir_filter && mc_load_ir_filter && mc_load_ir_sweep_filter && mc_ir_filter_info, "filter step (mc_load_ir_filter)"},
        {r.match && generated ? "match" : nullptr, matched, mc_default_ir_match && mc_load_ir_match && mc_load_ir_sweep_match && mc_ir_match_info && mc_ir_match_curve, "match step (mc_load_ir_match)"},
        {r.parts && generated ? "parts" : nullptr, parted, mc_default_ir_parts && mc_load_ir_parts && mc_load_ir_sweep_parts && mc_ir_parts_at && mc_ir_parts_info, "parts step (mc_load_ir_parts)"},
        {nullptr, tailed, mc_load_ir_tail && mc_load_ir_sweep_tail && mc_ir_tail_info, "tail step (mc_load_ir_tail)"},
        {nullptr, r.sweep.has_value(), mc_load_ir_sweep && mc_default_sweep && mc_ir_sweep_info, "sweep capture (mc_load_ir_sweep)"},
        {nullptr, generated, mc_synth_ir && mc_default_ir_synth && mc_ir_synth_info, "IR synthesis (mc_synth_ir)"},
        {nullptr, damped, mc_load_ir_damped && mc_default_ir_damp && mc_ir_damp_info, "IR damping (mc_load_ir_damped)"},
        {nullptr, true, mc_load_ir_shaped && mc_default_ir_shape && mc_ir_shape_info, "IR shaping (mc_load_ir_shaped)"},
        {nullptr, equalised, mc_load_ir_eq && mc_default_ir_eq && mc_ir_eq_response, "IR equalisation (mc_load_ir_eq)"},
    };
    for (const auto& c : capabilities) {
        if (c.dropped) Log::info(name, "IR %zu is generated: it has no %s step and is loaded as it is", idx, c.dropped);
        if (c.needed && !c.there) {
            Log::error("conv", "the engine has no %s", c.lacks);
            std::exit(2);
        }
    }

    // The rates of the call.  What is laid out in Hz (bands, crossovers, the tail's and the match's bands) or converts a second IR
    // needs the session's rate, and host frames that are not converted then count as being at it; otherwise the rates are passed
    // only to convert.  Seconds become frames at the session's rate.
    const unsigned session = r.sweep ? r.sweep->sweep.rate : generated ? r.synth->rate : r.sessionRate;
    const bool needsRate = equalised || damped || tailed || matched || (filtered && r.filter->rate && r.filter->rate != session);
    const unsigned irRate = needsRate && !r.irRate ? session : r.irRate, sessionRate = needsRate || r.irRate ? session : 0;
    if (irRate && irRate != sessionRate) Log::info(name, "IR %zu: %u Hz -> %u Hz", idx, irRate, sessionRate);

    // the settings as the engine's structs; a null pointer switches a step off
    const mc_ir_shape s = shapeArg(r.shape);
    mc_ir_eq eq;
    mc_ir_damp damp;
    mc_ir_phase phase;
    mc_ir_filter filter;
    mc_ir_match match;
    mc_ir_parts parts;
    if (minimum) phase = phaseArg(*r.phase);
    if (filtered) filter = filterArg(*r.filter, session);
    if (matched) match = matchArg(*r.match, session);
    if (parted) parts = partsArg(idx, *r.parts, (double)session, r.split);
    if (equalised) eq = eqArg(r.eq);
    if (damped) damp = dampArg(r.damp, (double)session);
    const mc_ir_eq* q = equalised ? &eq : nullptr;
    const mc_ir_damp* d = damped ? &damp : nullptr;
    const mc_ir_tail* t = tailed ? &*r.tail : nullptr;
    const mc_ir_phase* ph = minimum ? &phase : nullptr;
    const mc_ir_filter* fl = filtered ? &filter : nullptr;
    const mc_ir_match* mt = matched ? &match : nullptr;
    const mc_ir_parts* pt = parted ? &parts : nullptr;
    const float *flLr = filtered ? r.filter->lr.data() : nullptr, *mtLr = matched ? r.match->lr.data() : nullptr;
    const uint64_t flFrames = filtered ? r.filter->lr.size() / 2 : 0, mtFrames = matched ? r.match->lr.size() / 2 : 0;

    // the call: per source kind, the narrowest entry point that takes everything that is on
    if (generated) {  // (what the engine refuses of a generated IR is the index line's fault: a message and exit 2, no abort)
        const mc_ir_synth* y = &*r.synth;
        const mc_ir_room* room = r.room ? &*r.room : nullptr;
        const mc_ir_room_mics* mics = r.mics ? &*r.mics : nullptr;
        const mc_ir_room_bands* bands = r.bands ? &*r.bands : nullptr;
        const mc_ir_room_head* head = r.head ? &*r.head : nullptr;
        const int rc = head   ? mc_synth_ir_room_head(_engine, idx, r.nframes, y, room, mics, bands, head, &s, q, d, t)
                       : bands ? mc_synth_ir_room_bands(_engine, idx, r.nframes, y, room, mics, bands, &s, q, d, t)
                       : mics ? mc_synth_ir_room_mics(_engine, idx, r.nframes, y, room, mics, &s, q, d, t)
                       : room ? mc_synth_ir_room(_engine, idx, r.nframes, y, room, &s, q, d, t)
                       : r.plate ? mc_synth_ir_plate(_engine, idx, r.nframes, y, &*r.plate, &s, q, d, t)
                       : r.spring ? mc_synth_ir_spring(_engine, idx, r.nframes, y, &*r.spring, &s, q, d, t)
                              : mc_synth_ir(_engine, idx, r.nframes, y, &s, q, d);
        if (rc != MC_OK) {
            Log::error("conv", "IR %zu cannot be synthesised: %s", idx, mc_last_error());
            std::exit(2);
        }
    } else if (r.sweep) {  // (as for a generated IR: what the engine refuses is the index line's fault)
        const SweepLoad& w = *r.sweep;
        const int rc = pt   ? mc_load_ir_sweep_parts(_engine, idx, r.lr, r.frames, r.nframes, &w.sweep, w.offset, w.irFrames, &s, q, d, t, ph, fl, flLr, flFrames, mt, mtLr, mtFrames, pt)
                       : mt ? mc_load_ir_sweep_match(_engine, idx, r.lr, r.frames, r.nframes, &w.sweep, w.offset, w.irFrames, &s, q, d, t, ph, fl, flLr, flFrames, mt, mtLr, mtFrames)
                       : fl ? mc_load_ir_sweep_filter(_engine, idx, r.lr, r.frames, r.nframes, &w.sweep, w.offset, w.irFrames, &s, q, d, t, ph, fl, flLr, flFrames)
                       : ph ? mc_load_ir_sweep_phase(_engine, idx, r.lr, r.frames, r.nframes, &w.sweep, w.offset, w.irFrames, &s, q, d, t, ph)
                       : t  ? mc_load_ir_sweep_tail(_engine, idx, r.lr, r.frames, r.nframes, &w.sweep, w.offset, w.irFrames, &s, q, d, t)
                            : mc_load_ir_sweep(_engine, idx, r.lr, r.frames, r.nframes, &w.sweep, w.offset, w.irFrames, &s, q, d);
        if (rc != MC_OK) {
            Log::error("conv", "IR %zu cannot be captured: %s", idx, mc_last_error());
            std::exit(2);
        }
    } else if (pt || mt || fl || ph) {  // (what these steps refuse is the command line's fault: a message and exit 2, no abort)
        const int rc = pt   ? mc_load_ir_parts(_engine, idx, r.lr, r.frames, r.nframes, irRate, sessionRate, &s, q, d, t, ph, fl, flLr, flFrames, mt, mtLr, mtFrames, pt)
                       : mt ? mc_load_ir_match(_engine, idx, r.lr, r.frames, r.nframes, irRate, sessionRate, &s, q, d, t, ph, fl, flLr, flFrames, mt, mtLr, mtFrames)
                       : fl ? mc_load_ir_filter(_engine, idx, r.lr, r.frames, r.nframes, irRate, sessionRate, &s, q, d, t, ph, fl, flLr, flFrames)
                            : mc_load_ir_phase(_engine, idx, r.lr, r.frames, r.nframes, irRate, sessionRate, &s, q, d, t, ph);
        if (rc != MC_OK) {
            if (pt) Log::error("conv", "IR %zu cannot be split into parts: %s", idx, mc_last_error());
            else if (mt) Log::error("conv", "IR %zu cannot be matched to %s: %s", idx, r.match->path.c_str(), mc_last_error());
            else if (fl) Log::error("conv", "IR %zu cannot be filtered with %s: %s", idx, r.filter->path.c_str(), mc_last_error());
            else Log::error("conv", "IR %zu cannot be converted to minimum phase: %s", idx, mc_last_error());
            std::exit(2);
        }
    } else if (t)
        check(mc_load_ir_tail(_engine, idx, r.lr, r.frames, r.nframes, irRate, sessionRate, &s, q, d, t), "mc_load_ir_tail");
    else if (d)
        check(mc_load_ir_damped(_engine, idx, r.lr, r.frames, r.nframes, irRate, sessionRate, &s, q, d), "mc_load_ir_damped");
    else if (q)
        check(mc_load_ir_eq(_engine, idx, r.lr, r.frames, r.nframes, irRate, sessionRate, &s, q), "mc_load_ir_eq");
    else
        check(mc_load_ir_shaped(_engine, idx, r.lr, r.frames, r.nframes, irRate, sessionRate, &s), "mc_load_ir_shaped");

    // what was done: the source's lines, then one per step in the order the frames went through them
    if (r.plate) {
        double pi[8];
        check(mc_ir_plate_info(_engine, idx, pi), "mc_ir_plate_info");
        Log::info(name, "IR %zu plate: %llu modes from %.2f to %.2f Hz, %llu and %llu sounding, before frame %llu, kappa %.4f m^2/s", idx,
                  (unsigned long long)pi[0], pi[4], pi[5], (unsigned long long)pi[1], (unsigned long long)pi[2], (unsigned long long)pi[3], pi[6]);
    }
    if (r.spring) {
        double si[24];
        check(mc_ir_spring_info(_engine, idx, si), "mc_ir_spring_info");
        std::string delays;
        for (int k = 0; k < (int)si[3]; k++) {
            char one[64];
            std::snprintf(one, sizeof(one), "%s%llu/%llu", k ? ", " : "", (unsigned long long)si[8 + 2 * k], (unsigned long long)si[9 + 2 * k]);
            delays += one;
        }
        Log::info(name, "IR %zu spring: %llu points, K %llu (transition %.1f Hz), %llu sections, low-pass %s, %llu springs with delays %s frames (L/R), before frame %llu, alias bound %.1f dB",
                  idx, (unsigned long long)si[0], (unsigned long long)si[1], si[2], (unsigned long long)si[4], si[5] != 0.0 ? "in" : "out", (unsigned long long)si[3],
                  delays.c_str(), (unsigned long long)si[6], si[7]);
    }
    if (r.room) {
        double ri[8];
        check(mc_ir_room_info(_engine, idx, ri), "mc_ir_room_info");
        Log::info(name, "IR %zu room: order %d, %llu and %llu images before frame %llu, direct sound at %.2f and %.2f frames, complete up to frame %llu",
                  idx, (int)ri[0], (unsigned long long)ri[1], (unsigned long long)ri[2], (unsigned long long)ri[5], ri[3], ri[4],
                  (unsigned long long)ri[6]);
    }
    if (r.mics) {
        double mi[8];
        check(mc_ir_room_mics_info(_engine, idx, mi), "mc_ir_room_mics_info");
        Log::info(name, "IR %zu microphones: the direct sound leaves the source at %.4f and %.4f, is received at %.4f and %.4f, factors %.4f and %.4f",
                  idx, mi[0], mi[1], mi[2], mi[3], mi[4], mi[5]);
    }
    if (r.bands) {
        double bi[16];
        check(mc_ir_room_bands_info(_engine, idx, bi), "mc_ir_room_bands_info");
        std::string sabine, eyring;
        for (int j = 0; j < (int)bi[0]; j++) {
            char one[32];
            std::snprintf(one, sizeof(one), "%s%.3f", j ? " / " : "", bi[4 + j]);
            sabine += one;
            std::snprintf(one, sizeof(one), "%s%.3f", j ? " / " : "", bi[8 + j]);
            eyring += one;
        }
        Log::info(name, "IR %zu bands: %d, low to high Sabine %s s, Eyring %s s", idx, (int)bi[0], sabine.c_str(), eyring.c_str());
    }
    if (r.head) {
        double hi[12];
        check(mc_ir_room_head_info(_engine, idx, hi), "mc_ir_room_head_info");
        Log::info(name, "IR %zu head: the direct sound reaches the ears at %.2f and %.2f frames (right minus left %+.4f ms), %.1f and %.1f degrees off their "
                        "axes, shadow factors %+.4f and %+.4f, shelf corner %.0f Hz",
                  idx, hi[2], hi[3], hi[4] * 1e3, hi[5], hi[6], hi[7], hi[8], hi[9]);
    }
    if (generated) {
        double si[4];
        check(mc_ir_synth_info(_engine, idx, si), "mc_ir_synth_info");
        Log::info(name, "IR %zu synthesised: %llu frames, seed %llu, %d of %u reflections kept", idx, (unsigned long long)si[0],
                  (unsigned long long)r.synth->seed, (int)si[1], r.synth->n_early);
    }
    if (r.sweep) {
        double wi[4];
        check(mc_ir_sweep_info(_engine, idx, wi), "mc_ir_sweep_info");
        Log::info(name, "IR %zu captured: sweep %llu frames, recording %llu frames, %llu frames at offset %lld", idx, (unsigned long long)wi[0],
                  (unsigned long long)wi[1], (unsigned long long)wi[2], (long long)wi[3]);
    }
    if (t) {
        double ti[4];
        check(mc_ir_tail_info(_engine, idx, ti), "mc_ir_tail_info");
        std::string knees;
        for (uint32_t j = 0; j <= t->n_xovers; j++)
            knees += (j ? ", " : "") + (t->knee[j] == ~0ull ? std::string("none") : std::to_string((unsigned long long)t->knee[j]));
        Log::info(name, "IR %zu tail: %s, %d of %u bands at knees %s, %llu frames in, %llu out, first frame changed %llu", idx,
                  t->mode == MC_TAIL_CUT ? "cut" : "extended", (int)ti[0], t->n_xovers + 1, knees.c_str(), (unsigned long long)ti[1],
                  (unsigned long long)ti[2], (unsigned long long)ti[3]);
    }
    if (ph) {
        double pi[8];
        check(mc_ir_phase_info(_engine, idx, pi), "mc_ir_phase_info");
        const double removed = pi[4] - pi[5];
        Log::info(name, "IR %zu minimum phase: %llu frames through a transform of %llu points, delay removed %.1f frames (%.3f ms), %.4f dB kept, %llu and %llu bins at the floor",
                  idx, (unsigned long long)pi[0], (unsigned long long)pi[1], removed, samplerate ? 1000.0 * removed / (double)samplerate : 0.0,
                  pi[2] > 0.0 && pi[3] > 0.0 ? 10.0 * std::log10(pi[3] / pi[2]) : 0.0, (unsigned long long)pi[6], (unsigned long long)pi[7]);
    }
    if (fl) {
        double fi[10];
        check(mc_ir_filter_info(_engine, idx, fi), "mc_ir_filter_info");
        Log::info(name, "IR %zu %s %s: %llu frames and %llu filter frames through a transform of %llu points, %llu frames kept, level %+.2f dB, %.2f dB left behind, %llu and %llu bins regularised",
                  idx, r.filter->deconvolve ? "deconvolved by" : "convolved with", r.filter->path.c_str(), (unsigned long long)fi[0], (unsigned long long)fi[1],
                  (unsigned long long)fi[3], (unsigned long long)fi[2], fi[4] > 0.0 && fi[6] > 0.0 ? 10.0 * std::log10(fi[6] / fi[4]) : 0.0,
                  fi[6] > 0.0 && fi[7] > 0.0 ? std::max(-999.0, 10.0 * std::log10(fi[7] / fi[6])) : -999.0, (unsigned long long)fi[8], (unsigned long long)fi[9]);
    }
    if (mt) {
        double mi[12];
        check(mc_ir_match_info(_engine, idx, mi), "mc_ir_match_info");
        std::vector<double> hz(1024), before(2048), gain(2048);
        const int J = mc_ir_match_curve(_engine, idx, hz.data(), before.data(), gain.data(), 1024);
        if (J < 0) check(J, "mc_ir_match_curve");
        double least = 0.0, most = 0.0;
        for (int j = 0; j < 2 * J; j++) least = std::min(least, gain[j]), most = std::max(most, gain[j]);
        Log::info(name, "IR %zu matched to %s: %llu frames and %llu target frames through a transform of %llu points, %llu frames kept, %d points, gain %+.2f .. %+.2f dB, %llu clamped, level %+.2f dB",
                  idx, r.match->path.c_str(), (unsigned long long)mi[0], (unsigned long long)mi[1], (unsigned long long)mi[3], (unsigned long long)mi[2], J, least,
                  most, (unsigned long long)mi[11], mi[5] > 0.0 && mi[7] > 0.0 ? 10.0 * std::log10(mi[7] / mi[5]) : 0.0);
        if (_irMatchReport)
            for (int j = 0; j < J; j++)
                Log::info(name, "IR %zu match %.3f Hz: before %+.4f %+.4f dB, gain %+.4f %+.4f dB", idx, hz[j], before[2 * j], before[2 * j + 1], gain[2 * j],
                          gain[2 * j + 1]);
    }
    if (pt) {
        double pi[10];
        check(mc_ir_parts_info(_engine, idx, pi), "mc_ir_parts_info");
        const double rest = pi[5] + pi[6];
        Log::info(name, "IR %zu parts: %llu frames in, %llu out, direct to %llu, early to %llu%s, energies %.6e / %.6e / %.6e, direct to reverberant %+.2f dB, level %+.2f dB, %llu contributions lost (%.6e)",
                  idx, (unsigned long long)pi[0], (unsigned long long)pi[1], (unsigned long long)pi[2], (unsigned long long)pi[3],
                  r.split ? " (the mixing tap)" : "", pi[4], pi[5], pi[6], pi[4] > 0.0 && rest > 0.0 ? 10.0 * std::log10(pi[4] / rest) : 0.0,
                  pi[4] + rest > 0.0 && pi[7] > 0.0 ? 10.0 * std::log10(pi[7] / (pi[4] + rest)) : 0.0, (unsigned long long)pi[9], pi[8]);
    }
    double info[8];
    check(mc_ir_shape_info(_engine, idx, info), "mc_ir_shape_info");
    Log::info(name, "IR %zu shaped: onset %llu, first kept frame %llu, %llu taps, gain %+.2f dB", idx, (unsigned long long)info[1],
              (unsigned long long)info[2], (unsigned long long)info[3], 20.0 * std::log10(info[4]));
    if (q) {
        const double hz = 1000.0;
        double db = 0.0;
        check(mc_ir_eq_response(q, sessionRate, &hz, 1, &db), "mc_ir_eq_response");
        Log::info(name, "IR %zu equalised: %d bands, %+.2f dB at 1 kHz", idx, (int)info[7], db);
    }
    if (d) {
        double di[4];
        check(mc_ir_damp_info(_engine, idx, di), "mc_ir_damp_info");
        std::string decays;
        for (uint32_t j = 0; j <= d->n_xovers; j++) decays += (j ? ", " : "") + std::to_string((unsigned long long)d->decay_t60[j]);
        Log::info(name, "IR %zu damped: %d crossovers, origin %llu, %d bands with a decay (%s frames)", idx, (int)di[0], (unsigned long long)di[1],
                  (int)di[2], decays.c_str());
    }
}

void Convolution::setIrDecayReport(bool on, const std::vector<float>& bands) {
    if (on && _group) {
        Log::error("conv", "the IR decay report is not available with several devices (mc_ir_decay is single-engine)");
        std::exit(2);
    }
    if (bands.size() > MC_DECAY_MAX_BANDS) {
        Log::error("conv", "%zu decay bands, at most %d", bands.size(), MC_DECAY_MAX_BANDS);
        std::exit(2);
    }
    _decayReport = on;
    _decayBands = bands;
}

void Convolution::setIrRt60(double seconds) {
    if (seconds > 0.0 && _group) {
        Log::error("conv", "aiming IRs at a decay time is not available with several devices (mc_ir_decay is single-engine)");
        std::exit(2);
    }
    _rt60 = seconds > 0.0 ? seconds : 0.0;
}

uint64_t Convolution::decayForRt60(double measured, double target, double rate) {
    if (!(std::isfinite(measured) && std::isfinite(target) && target > 0.0 && target < measured)) return 0;
    return (uint64_t)std::nearbyint(rate / (1.0 / target - 1.0 / measured));
}

Convolution::Decay Convolution::irDecay(size_t idx, const DecayQuery& query) {
    if (!mc_ir_decay || !mc_default_decay_query) {
        Log::error("conv", "the engine has no decay measurement (mc_ir_decay)");
        std::exit(2);
    }
    if (query.bands.size() > MC_DECAY_MAX_BANDS) {
        Log::error("conv", "%zu decay bands, at most %d", query.bands.size(), MC_DECAY_MAX_BANDS);
        std::exit(2);
    }
    mc_decay_query q;
    mc_default_decay_query(&q);
    q.rate = query.rate ? query.rate : (uint32_t)samplerate;
    q.n_bands = (uint32_t)query.bands.size();
    for (size_t k = 0; k < query.bands.size(); k++) q.centre_hz[k] = query.bands[k];
    q.q = query.q;
    q.onset_db = query.onsetDb;
    q.end = query.end;
    q.curve_points = query.curvePoints;
    Decay d;
    d.rows.resize((1 + query.bands.size()) * 3 * 8);
    d.curve.resize((1 + query.bands.size()) * 3 * query.curvePoints);
    uint64_t info[2] = {0, 0};
    check(mc_ir_decay(_engine, idx, &q, d.rows.data(), d.curve.empty() ? nullptr : d.curve.data(), info), "mc_ir_decay");
    d.origin = info[0];
    d.taps = info[1];
    return d;
}

namespace {
// a number with `decimals` places, NaN as "nan" whatever its sign
std::string places(double v, int decimals) {
    if (std::isnan(v)) return "nan";
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%.*f", decimals, v);
    return buf;
}
}  // namespace

void Convolution::reportDecay(size_t idx) {
    DecayQuery query;
    query.bands = _decayBands;
    const Decay d = irDecay(idx, query);
    for (size_t b = 0; b <= _decayBands.size(); b++) {
        char head[64] = "";
        if (b) std::snprintf(head, sizeof(head), " band %g Hz", (double)_decayBands[b - 1]);
        const auto v = [&](Decay::Field f, int decimals, double scale = 1.0) { return places(scale * d.at(b, Decay::LR, f), decimals); };
        Log::info(name, "IR %zu%s decay: origin %llu, EDT %s s, T20 %s s, T30 %s s, C50 %s dB, C80 %s dB, Ts %s ms", idx, head,
                  (unsigned long long)d.origin, v(Decay::Edt, 4).c_str(), v(Decay::T20, 4).c_str(), v(Decay::T30, 4).c_str(), v(Decay::C50, 2).c_str(),
                  v(Decay::C80, 2).c_str(), v(Decay::Ts, 2, 1000.0).c_str());
    }
}

// broadband LR T30 of a loaded IR, T20 when the curve does not reach -35 dB (NaN when it does not reach -25 dB either)
static double measuredRt(Convolution& c, size_t idx) {
    const Convolution::Decay d = c.irDecay(idx, Convolution::DecayQuery());
    const double t30 = d.at(0, Convolution::Decay::LR, Convolution::Decay::T30);
    return std::isnan(t30) ? d.at(0, Convolution::Decay::LR, Convolution::Decay::T20) : t30;
}

void Convolution::aimRt60(const IrLoadRequest& loaded) {
    const double measured = measuredRt(*this, loaded.idx);
    if (std::isnan(measured)) {
        Log::warn(name, "IR %zu rt60: its decay curve does not reach -25 dB, left as it is", loaded.idx);
        return;
    }
    const uint64_t fit = decayForRt60(measured, _rt60, (double)samplerate);
    if (!fit) {
        Log::info(name, "IR %zu rt60: target %.4f s is not below the measured %.4f s, left as it is", loaded.idx, _rt60, measured);
        return;
    }
    // slopes add: 1 / d = 1 / d_user + 1 / d_fit
    IrLoadRequest again = loaded;  // (the measured tail and split included)
    IrShape& shape = again.shape;
    shape.decayT60 = shape.decayT60 ? (uint64_t)std::nearbyint(1.0 / (1.0 / (double)shape.decayT60 + 1.0 / (double)fit)) : fit;
    if (!shape.decayT60) shape.decayT60 = 1;
    loadIr(again);
    Log::info(name, "IR %zu rt60: measured %.4f s, decay %llu frames, now %s s", loaded.idx, measured, (unsigned long long)shape.decayT60,
              places(measuredRt(*this, loaded.idx), 4).c_str());
}

void Convolution::setIrFloorReport(bool on) {
    if (on && _group) {
        Log::error("conv", "the IR floor report is not available with several devices (mc_ir_floor is single-engine)");
        std::exit(2);
    }
    _floorReport = on;
}

void Convolution::setIrFloorXovers(const std::vector<float>& xovers) {
    if (xovers.size() > MC_FLOOR_MAX_XOVERS) {
        Log::error("conv", "%zu floor crossovers, at most %d", xovers.size(), MC_FLOOR_MAX_XOVERS);
        std::exit(2);
    }
    _floorXovers = xovers;
}

void Convolution::setIrTail(const IrTail& tail) {
    if (tail.mode != IrTail::Off && _group) {
        Log::error("conv", "the IR tail step is not available with several devices (mc_load_ir_tail is single-engine)");
        std::exit(2);
    }
    _irTail = tail;
}

void Convolution::setIrPhase(const IrPhase& phase) {
    if (phase.minimum && _group) {
        Log::error("conv", "the IR phase step is not available with several devices (mc_load_ir_phase is single-engine)");
        std::exit(2);
    }
    _irPhase = phase;
}

void Convolution::setIrFilter(const IrFilter& filter) {
    if (filter.on && _group) {
        Log::error("conv", "the IR filter step is not available with several devices (mc_load_ir_filter is single-engine)");
        std::exit(2);
    }
    _irFilter = filter;
}

void Convolution::setIrParts(const IrParts& parts) {
    if (parts.on && _group) {
        Log::error("conv", "the IR parts step is not available with several devices (mc_load_ir_parts is single-engine)");
        std::exit(2);
    }
    _irParts = parts;
}

// Loads p with every step but the parts (the measured tail included) and with no shape, EQ or damping, measures its echo density
// and returns the boundaries its final load goes through; nothing for a generated IR, which has no parts step
std::optional<Convolution::PartsSplit> Convolution::measureParts(const PendingIr& p, const std::optional<mc_ir_tail>& tail) {
    if (!mc_default_ir_parts || !mc_load_ir_parts || !mc_load_ir_sweep_parts || !mc_ir_parts_at || !mc_ir_parts_info) {
        Log::error("conv", "the engine has no parts step (mc_load_ir_parts)");
        std::exit(2);
    }
    if (p.generated) return std::nullopt;  // (loadIr says that it has no parts step)
    IrLoadRequest raw = requestFor(p);
    raw.tail = tail;
    raw.parts = nullptr;
    raw.shape = IrShape(), raw.eq = IrEq(), raw.damp = IrDamp();
    loadIr(raw);
    const Density d = irDensity(p.idx, _densityQuery);
    PartsSplit split{d.origin, 0};
    if (d.at(Decay::LR, Density::Status) != 0.0) {
        split.mix = split.onset + (uint64_t)std::nearbyint(0.08 * (double)samplerate);
        Log::warn(name, "IR %zu parts: the echo density never reaches 1 (largest %s), the early part ends 80 ms after the onset at frame %llu", p.idx,
                  places(d.at(Decay::LR, Density::Max), 3).c_str(), (unsigned long long)split.onset);
    } else {
        split.mix = std::max<uint64_t>((uint64_t)d.at(Decay::LR, Density::Mix), split.onset);
        Log::info(name, "IR %zu parts: onset at frame %llu, the early part ends at the mixing tap %llu", p.idx, (unsigned long long)split.onset,
                  (unsigned long long)split.mix);
    }
    return split;
}

void Convolution::setIrMatch(const IrMatch& match, bool report) {
    if (match.on && _group) {
        Log::error("conv", "the IR match step is not available with several devices (mc_load_ir_match is single-engine)");
        std::exit(2);
    }
    _irMatch = match;
    _irMatchReport = report;
}

Convolution::Floor Convolution::irFloor(size_t idx, const std::vector<float>& xovers, unsigned rate) {
    if (!mc_ir_floor || !mc_default_floor_query) {
        Log::error("conv", "the engine has no floor measurement (mc_ir_floor)");
        std::exit(2);
    }
    if (xovers.size() > MC_FLOOR_MAX_XOVERS) {
        Log::error("conv", "%zu floor crossovers, at most %d", xovers.size(), MC_FLOOR_MAX_XOVERS);
        std::exit(2);
    }
    Floor f;
    mc_default_floor_query(&f.query);
    f.query.rate = rate ? rate : (uint32_t)samplerate;
    f.query.n_xovers = (uint32_t)xovers.size();
    for (size_t k = 0; k < xovers.size(); k++) f.query.xover_hz[k] = xovers[k];
    f.rows.resize((1 + (xovers.empty() ? 0 : xovers.size() + 1)) * 3 * 8);
    uint64_t info[2] = {0, 0};
    if (mc_ir_floor(_engine, idx, &f.query, f.rows.data(), info) != MC_OK) {  // (crossovers the rate does not allow: the command line's fault)
        Log::error("conv", "IR %zu: the floor cannot be measured: %s", idx, mc_last_error());
        std::exit(2);
    }
    f.origin = info[0];
    f.taps = info[1];
    return f;
}

void Convolution::reportFloor(size_t idx) {
    const Floor f = irFloor(idx, _floorXovers);
    for (size_t g = 0; g < f.groups(); g++) {
        char head[32] = "";
        if (g) std::snprintf(head, sizeof(head), " band %zu", g - 1);
        const auto v = [&](Floor::Field fld, int decimals) { return places(f.at(g, Decay::LR, fld), decimals); };
        const double nz = f.at(g, Decay::LR, Floor::Noise);
        Log::info(name, "IR %zu%s floor: origin %llu, knee %s, T %s s, noise %s dB, peak to noise %s dB, interval %s, status %d", idx, head,
                  (unsigned long long)f.origin, v(Floor::Knee, 1).c_str(), v(Floor::T, 4).c_str(), places(10.0 * std::log10(nz), 2).c_str(),
                  v(Floor::PeakToNoise, 2).c_str(), v(Floor::Interval, 0).c_str(), (int)f.at(g, Decay::LR, Floor::Status));
    }
}

// Loads p as it is (no shape, EQ or damping: the frames at the client's rate), measures its floor and returns the tail step its
// final load goes through; nothing for an IR that is left as it is
std::optional<mc_ir_tail> Convolution::measureTail(const PendingIr& p) {
    if (!mc_ir_tail_from_floor || !mc_default_ir_tail || !mc_load_ir_tail) {
        Log::error("conv", "the engine has no tail step (mc_load_ir_tail)");
        std::exit(2);
    }
    if (p.generated && !p.roomed && !p.plated && !p.sprung) {
        Log::info(name, "IR %zu tail: a generated IR has no floor, left as it is", p.idx);
        return std::nullopt;
    }
    IrLoadRequest raw = requestFor(p);
    raw.shape = IrShape(), raw.eq = IrEq(), raw.damp = IrDamp();
    raw.phase = nullptr, raw.filter = nullptr, raw.match = nullptr;  // (the floor is that of the frames the tail step will see: before the steps after it)
    // A known divergence from that, and from what DESIGN.md says: raw.parts stays, so with the parts step on the floor is measured
    // on frames that went through it, although it runs after the tail.  Kept as the host has behaved since the parts step came.
    loadIr(raw);
    const Floor f = irFloor(p.idx, _floorXovers);
    const double need = (double)f.query.margin_db + (double)f.query.span_db, ptn = f.at(0, Decay::LR, Floor::PeakToNoise);
    if (f.at(0, Decay::LR, Floor::Status) != 0.0 || !(ptn >= need)) {
        Log::info(name, "IR %zu tail: peak to noise %s dB (status %d) is under %g dB, left as it is", p.idx, places(ptn, 2).c_str(),
                  (int)f.at(0, Decay::LR, Floor::Status), need);
        return std::nullopt;
    }
    mc_ir_tail tail;
    mc_default_ir_tail(&tail);
    const uint64_t info[2] = {f.origin, f.taps};
    check(mc_ir_tail_from_floor(&f.query, f.rows.data(), info, 0, &tail), "mc_ir_tail_from_floor");
    tail.mode = _irTail.mode == IrTail::Cut ? MC_TAIL_CUT : MC_TAIL_EXTEND;
    tail.fade = (uint32_t)std::nearbyint(_irTail.fadeSeconds * (double)samplerate);
    tail.length = (uint64_t)std::nearbyint(_irTail.lengthSeconds * (double)samplerate);
    tail.seed = _irTail.seed;
    tail.width = _irTail.width;
    if (_irTail.widthFromIacc) {
        if (!mc_ir_tail_width_from_iacc) {
            Log::error("conv", "the engine cannot take a width from an IACC (mc_ir_tail_width_from_iacc)");
            std::exit(2);
        }
        IaccQuery broadband = _iaccQuery;  // (the lag of the command line; the width is read from the broadband group alone)
        broadband.bands.clear();
        const Iacc a = irIacc(p.idx, broadband);
        const double rho = a.at(0, Iacc::Late, Iacc::Iacf0);
        if (a.at(0, Iacc::Late, Iacc::Status) != 0.0)
            Log::warn(name, "IR %zu tail: the late window from tap %llu has no correlation to read (status 1), the width stays %.9g", p.idx,
                      (unsigned long long)a.split, (double)tail.width);
        else {
            check(mc_ir_tail_width_from_iacc(&tail, rho), "mc_ir_tail_width_from_iacc");
            Log::info(name, "IR %zu tail: width %.9g from the late IACF(0) %.9f", p.idx, (double)tail.width, rho);
        }
    }
    if (!_irTail.kneeAtMix) return tail;
    if (!mc_ir_tail_move_knee) {
        Log::error("conv", "the engine cannot move a knee (mc_ir_tail_move_knee)");
        std::exit(2);
    }
    const Density d = irDensity(p.idx, _densityQuery);
    if (d.at(Decay::LR, Density::Status) != 0.0) {
        Log::warn(name, "IR %zu tail: the echo density never reaches 1 (largest %s), the knees stay at the floor's", p.idx,
                  places(d.at(Decay::LR, Density::Max), 3).c_str());
        return tail;
    }
    const uint64_t mix = (uint64_t)d.at(Decay::LR, Density::Mix);
    for (uint32_t j = 0; j <= tail.n_xovers; j++)
        if (tail.knee[j] != ~0ull) check(mc_ir_tail_move_knee(&tail, j, mix), "mc_ir_tail_move_knee");
    Log::info(name, "IR %zu tail: knees moved to the mixing tap %llu", p.idx, (unsigned long long)mix);
    return tail;
}

void Convolution::setIrDensityReport(bool on, const DensityQuery& query) {
    if (on && _group) {
        Log::error("conv", "the IR density report is not available with several devices (mc_ir_density is single-engine)");
        std::exit(2);
    }
    _densityReport = on;
    _densityQuery = query;
}

Convolution::Density Convolution::irDensity(size_t idx, const DensityQuery& query) {
    if (!mc_ir_density || !mc_default_density_query) {
        Log::error("conv", "the engine has no density measurement (mc_ir_density)");
        std::exit(2);
    }
    const double rate = (double)samplerate;
    mc_density_query q;
    mc_default_density_query(&q);
    q.rate = (uint32_t)samplerate;
    if (query.windowSeconds > 0.0) q.half = (uint32_t)std::min(std::floor(query.windowSeconds * rate / 2.0 + 0.5), 4294967295.0);
    if (query.hopSeconds > 0.0) q.hop = (uint32_t)std::min(std::max(std::nearbyint(query.hopSeconds * rate), 1.0), 4294967295.0);
    double t60 = query.t60Seconds;
    if (query.autoT60) t60 = irDecay(idx, DecayQuery()).at(0, Decay::LR, Decay::T30);  // (NaN: nothing is undone)
    if (t60 > 0.0) q.decay_t60 = (uint64_t)std::max(std::nearbyint(t60 * rate), 1.0);
    Density d;
    uint64_t info[3] = {0, 0, 0};
    if (mc_ir_density(_engine, idx, &q, d.rows, nullptr, info) != MC_OK) {  // (a window or a hop the engine does not take: the command line's fault)
        Log::error("conv", "IR %zu: the density cannot be measured: %s", idx, mc_last_error());
        std::exit(2);
    }
    d.origin = info[0], d.taps = info[1], d.centres = info[2];
    return d;
}

void Convolution::reportDensity(size_t idx) {
    const Density d = irDensity(idx, _densityQuery);
    const auto v = [&](Density::Field f, int decimals) { return places(d.at(Decay::LR, f), decimals); };
    Log::info(name, "IR %zu density: origin %llu, mixing %s (%s s), first %s, max %s at %s, after %s, silent %s, status %d", idx,
              (unsigned long long)d.origin, v(Density::Mix, 0).c_str(), v(Density::MixSeconds, 4).c_str(), v(Density::First, 3).c_str(),
              v(Density::Max, 3).c_str(), v(Density::MaxTap, 0).c_str(), v(Density::MeanAfter, 3).c_str(), v(Density::Silent, 0).c_str(),
              (int)d.at(Decay::LR, Density::Status));
}

void Convolution::setIrIaccReport(bool on, const IaccQuery& query) {
    if (on && _group) {
        Log::error("conv", "the IR IACC report is not available with several devices (mc_ir_iacc is single-engine)");
        std::exit(2);
    }
    _iaccReport = on;
    _iaccQuery = query;
}

Convolution::Iacc Convolution::irIacc(size_t idx, const IaccQuery& query) {
    if (!mc_ir_iacc || !mc_default_iacc_query) {
        Log::error("conv", "the engine has no IACC measurement (mc_ir_iacc)");
        std::exit(2);
    }
    const double rate = (double)samplerate;
    mc_iacc_query q;
    mc_default_iacc_query(&q);
    q.rate = (uint32_t)samplerate;
    q.max_lag = (uint32_t)std::floor((query.lagGiven ? query.lagSeconds : 0.001) * rate + 0.5);
    q.n_bands = (uint32_t)query.bands.size();
    for (size_t k = 0; k < query.bands.size(); k++) q.centre_hz[k] = query.bands[k];
    Iacc a;
    a.rows.resize((1 + query.bands.size()) * 3 * 8);
    uint64_t info[3] = {0, 0, 0};
    if (mc_ir_iacc(_engine, idx, &q, a.rows.data(), nullptr, info) != MC_OK) {  // (a lag or a band the engine does not take: the command line's fault)
        Log::error("conv", "IR %zu: the IACC cannot be measured: %s", idx, mc_last_error());
        std::exit(2);
    }
    a.origin = info[0], a.taps = info[1], a.split = info[2], a.maxLag = q.max_lag;
    return a;
}

void Convolution::reportIacc(size_t idx) {
    static const char* const window[3] = {"early", "late", "all"};
    const Iacc a = irIacc(idx, _iaccQuery);
    for (size_t g = 0; g <= _iaccQuery.bands.size(); g++)
        for (int w = 0; w < 3; w++) {
            if (g && w != Iacc::All) continue;  // (a band: the whole IR only)
            char head[64] = "";
            if (g) std::snprintf(head, sizeof(head), " band %g Hz", (double)_iaccQuery.bands[g - 1]);
            const auto v = [&](Iacc::Field f, int decimals, double scale = 1.0) { return places(scale * a.at(g, (Iacc::Window)w, f), decimals); };
            Log::info(name, "IR %zu%s iacc %s: origin %llu, IACC %s at %s taps (%s ms), IACF(0) %s, level %s dB, status %d", idx, head, window[w],
                      (unsigned long long)a.origin, v(Iacc::Peak, 4).c_str(), v(Iacc::Lag, 0).c_str(), v(Iacc::Lag, 3, 1000.0 / (double)samplerate).c_str(),
                      v(Iacc::Iacf0, 4).c_str(), v(Iacc::LevelDb, 2).c_str(), (int)a.at(g, (Iacc::Window)w, Iacc::Status));
        }
}

void Convolution::setIrStiReport(bool on, const StiQuery& query) {
    if (on && _group) {
        Log::error("conv", "the IR STI report is not available with several devices (mc_ir_sti is single-engine)");
        std::exit(2);
    }
    _stiReport = on;
    _stiQuery = query;
}

Convolution::Sti Convolution::irSti(size_t idx, const StiQuery& query) {
    if (!mc_ir_sti || !mc_default_sti_query) {
        Log::error("conv", "the engine has no STI measurement (mc_ir_sti)");
        std::exit(2);
    }
    mc_sti_query q;
    mc_default_sti_query(&q);  // (the seven octaves, IEC 60268-16's modulation frequencies and weights)
    q.rate = (uint32_t)samplerate;
    if (!query.snrDb.empty()) {
        q.flags |= MC_STI_SNR;
        for (size_t b = 0; b < query.snrDb.size() && b < MC_STI_MAX_BANDS; b++) q.snr_db[b] = query.snrDb[b];
    }
    Sti s;
    s.bands = q.n_bands;
    s.rows.resize((1 + (size_t)q.n_bands) * 3 * 4);
    std::vector<double> mtf((1 + (size_t)q.n_bands) * 3 * q.n_mod);
    uint64_t info[2] = {0, 0};
    if (mc_ir_sti(_engine, idx, &q, s.rows.data(), mtf.data(), s.sti, info) != MC_OK) {  // (a rate that cannot hold the 8 kHz octave)
        Log::error("conv", "IR %zu: the STI cannot be measured: %s", idx, mc_last_error());
        std::exit(2);
    }
    s.origin = info[0], s.taps = info[1];
    return s;
}

void Convolution::reportSti(size_t idx) {
    static const char* const set[3] = {"L", "R", "LR"};
    const Sti s = irSti(idx, _stiQuery);
    for (int k = 0; k < 3; k++) {
        std::string mti;
        int status = 0;
        for (size_t b = 1; b <= s.bands; b++) {
            mti += " " + places(s.at(b, (Decay::Set)k, Sti::Mti), 4);
            if (s.at(b, (Decay::Set)k, Sti::Status) != 0.0) status = 1;
        }
        Log::info(name, "IR %zu sti %s: origin %llu, STI %s (%s), MTI%s, status %d", idx, set[k], (unsigned long long)s.origin, places(s.sti[k], 4).c_str(),
                  stiRating(s.sti[k]), mti.c_str(), status);
    }
}

void Convolution::setIrResponseReport(bool on, const ResponseQuery& query) {
    if (on && _group) {
        Log::error("conv", "the IR response report is not available with several devices (mc_ir_response is single-engine)");
        std::exit(2);
    }
    _responseReport = on;
    _responseQuery = query;
}

Convolution::Response Convolution::irResponse(size_t idx, const ResponseQuery& query) {
    if (!mc_ir_response || !mc_default_response_query || !mc_response_grid || !mc_response_smooth) {
        Log::error("conv", "the engine has no response measurement (mc_ir_response)");
        std::exit(2);
    }
    const double rate = (double)samplerate;
    Response r;
    r.hz.resize(MC_RSP_MAX_FREQ);
    const int n = mc_response_grid(20.0, std::min(20000.0, 0.45 * rate), 24, r.hz.data(), (uint32_t)r.hz.size());
    mc_response_query q;
    mc_default_response_query(&q);
    q.rate = (uint32_t)samplerate;
    q.n_freq = n > 0 ? (uint32_t)n : 0;
    r.hz.resize(q.n_freq);
    r.resp.resize((size_t)2 * q.n_freq * 3);
    r.smoothed.resize((size_t)2 * q.n_freq);
    uint64_t spans[2] = {0, 0}, info[2] = {0, 0};
    if (mc_ir_response(_engine, idx, &q, r.hz.data(), nullptr, r.resp.data(), r.rows, spans, info) != MC_OK) {  // (a rate the engine does not take)
        Log::error("conv", "IR %zu: the response cannot be measured: %s", idx, mc_last_error());
        std::exit(2);
    }
    r.origin = info[0], r.taps = info[1];
    std::vector<double> power(q.n_freq);
    for (int c = 0; c < 2; c++) {
        for (size_t f = 0; f < q.n_freq; f++) power[f] = r.re(c, f) * r.re(c, f) + r.im(c, f) * r.im(c, f);
        if (mc_response_smooth(r.hz.data(), power.data(), q.n_freq, query.smoothOctaves, r.smoothed.data() + (size_t)c * q.n_freq) != MC_OK) {
            Log::error("conv", "IR %zu: the response cannot be smoothed: %s", idx, mc_last_error());
            std::exit(2);
        }
    }
    return r;
}

size_t Convolution::Response::nearest(double f) const {
    const long i = std::lround(24.0 * std::log2(f / 20.0));  // (the grid is 20 2^(i / 24))
    return (size_t)std::min<long>(std::max<long>(i, 0), (long)hz.size() - 1);
}

void Convolution::reportResponse(size_t idx) {
    static const char* const channel[2] = {"L", "R"};
    static const double centre[10] = {31.5, 63.0, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0, 16000.0};
    const Response r = irResponse(idx, _responseQuery);
    const double nan = std::numeric_limits<double>::quiet_NaN(), top = 0.45 * (double)samplerate;
    const size_t k1 = r.nearest(1000.0);
    for (int c = 0; c < 2; c++) {
        const bool bad = r.rows[4 * c + 2] != 0.0;
        const auto db = [&](size_t f) { return bad ? nan : 10.0 * std::log10(r.smoothed[(size_t)c * r.hz.size() + f]); };
        std::string levels;
        for (double f : centre)
            if (f < top) levels += " " + places(db(r.nearest(f)) - db(k1), 2);
        Log::info(name, "IR %zu response %s: origin %llu, 1 kHz level %s dB, octaves%s, delay at 1 kHz %s ms, status %d", idx, channel[c],
                  (unsigned long long)r.origin, places(db(k1), 2).c_str(), levels.c_str(), places(r.delay(c, k1) * 1000.0 / (double)samplerate, 3).c_str(),
                  bad ? 1 : 0);
    }
}

mc_ir_synth Convolution::synthFrames(const IrSynth& y, double rate) {
    const auto frames = [&](double seconds) { return (uint64_t)std::nearbyint(seconds * rate); };
    mc_ir_synth s;
    mc_default_ir_synth(&s);
    s.frames = frames(y.lengthSeconds);
    s.t60 = frames(y.t60Seconds);
    s.seed = y.seed;
    s.late_start = frames(y.startSeconds);
    s.build_up = (uint32_t)std::min<uint64_t>(frames(y.buildUpSeconds), 0xffffffffull);
    s.late_gain = y.late;
    s.direct = y.direct;
    s.n_early = y.early;
    s.early_first = frames(y.earlyFirstSeconds);
    s.early_last = frames(y.earlyLastSeconds);
    s.early_gain = y.earlyGain;
    s.width = y.width;
    s.rate = (uint32_t)rate;
    return s;
}

mc_ir_room Convolution::roomFrames(const IrRoom& room, double rate) {
    mc_ir_room r;
    mc_default_ir_room(&r);
    for (int a = 0; a < 3; a++) r.size_m[a] = room.size[a], r.source_m[a] = room.source[a], r.receiver_m[a] = room.receiver[a];
    for (int w = 0; w < 6; w++) r.beta[w] = room.beta[w];
    r.spacing_m = room.spacing;
    r.axis = room.axis;
    r.speed = room.speed;
    r.gain = room.gain;
    r.order = room.order;
    r.last = (uint64_t)std::nearbyint(room.lastSeconds * rate);
    return r;
}

mc_ir_room_mics Convolution::roomMics(const IrRoom& room) {
    mc_ir_room_mics m;
    mc_default_ir_room_mics(&m);
    for (int c = 0; c < 2; c++) m.mic_pattern[c] = room.micPattern[c], m.mic_az_deg[c] = room.micAim[c], m.mic_el_deg[c] = room.micTilt[c];
    m.src_pattern = room.sourcePattern;
    m.src_az_deg = room.sourceAim;
    m.src_el_deg = room.sourceTilt;
    return m;
}

mc_ir_room_bands Convolution::roomBands(const IrRoom& room) {
    mc_ir_room_bands b;
    mc_default_ir_room_bands(&b);
    b.n_xovers = room.nXovers;
    for (uint32_t k = 0; k < room.nXovers; k++) b.xover_hz[k] = room.xovers[k];
    for (uint32_t j = 0; j <= room.nXovers; j++) {
        for (int w = 0; w < 6; w++) b.beta[j][w] = room.nBetas ? room.betas[j] : room.beta[w];
        b.air_db_per_m[j] = room.air[room.nAir > 1 ? j : 0];
    }
    return b;
}

mc_ir_room_head Convolution::roomHead(const IrRoom& room) {
    mc_ir_room_head h;
    mc_default_ir_room_head(&h);
    h.radius_m = room.headRadius;
    h.facing_az_deg = room.headFacing;
    h.ear_deg = room.headEars;
    h.shadow = room.headShadow;
    return h;
}

void Convolution::prepareRoom(size_t idx, const IrRoom& room, size_t nframes) {
    if (_group) {
        Log::error("conv", "room rendering is not available with several devices (mc_synth_ir_room is single-engine)");
        std::exit(2);
    }
    PendingIr& p = pend(idx, nframes);  // (rendered by onStart(), once the client's rate is known)
    p.generated = p.roomed = true;
    p.synth = room.late;
    p.room = room;
}

mc_ir_plate Convolution::plateFrames(const IrPlate& plate, double rate) {
    mc_ir_plate p;
    mc_default_ir_plate(&p);
    for (int a = 0; a < 2; a++) {
        p.size_m[a] = plate.size[a], p.driver_m[a] = plate.driver[a], p.t60_s[a] = plate.t60[a];
        for (int c = 0; c < 2; c++) p.pickup_m[c][a] = plate.pickup[c][a];
    }
    p.thickness_mm = plate.thickness;
    p.young_gpa = plate.material[0], p.density = plate.material[1], p.poisson = plate.material[2];
    p.low_hz = plate.low, p.high_hz = plate.high;
    p.damp_hz = plate.damp;
    p.gain = plate.gain;
    p.last = (uint64_t)std::nearbyint(plate.lastSeconds * rate);
    return p;
}

void Convolution::preparePlate(size_t idx, const IrPlate& plate, size_t nframes) {
    if (_group) {
        Log::error("conv", "plate synthesis is not available with several devices (mc_synth_ir_plate is single-engine)");
        std::exit(2);
    }
    PendingIr& p = pend(idx, nframes);  // (generated by onStart(), once the client's rate is known)
    p.generated = p.plated = true;
    p.synth = IrSynth();
    p.synth.lengthSeconds = plate.lengthSeconds;
    p.synth.late = 0.0f;  // (the plate alone: no late field under it)
    p.plate = plate;
}

mc_ir_spring Convolution::springFrames(const IrSpring& spring, double rate) {
    mc_ir_spring s;
    mc_default_ir_spring(&s);
    s.sections = spring.sections;
    s.transition_hz = spring.transition, s.dispersion = spring.dispersion;
    for (int k = 0; k < 3; k++) s.delay_ms[k] = spring.delayMs[k];
    s.t60_s = spring.t60, s.damping = spring.damping;
    s.lowpass_order = spring.lowpass;
    s.high_gain = spring.high, s.high_sections = spring.highSections;
    s.high_dispersion = spring.highDispersion, s.high_delay = spring.highDelay, s.high_t60_s = spring.highT60;
    s.stereo = spring.stereo, s.gain = spring.gain;
    s.log2_points = spring.points;
    s.last = (uint64_t)std::nearbyint(spring.lastSeconds * rate);
    return s;
}

void Convolution::prepareSpring(size_t idx, const IrSpring& spring, size_t nframes) {
    if (_group) {
        Log::error("conv", "spring synthesis is not available with several devices (mc_synth_ir_spring is single-engine)");
        std::exit(2);
    }
    PendingIr& p = pend(idx, nframes);  // (generated by onStart(), once the client's rate is known)
    p.generated = p.sprung = true;
    p.synth = IrSynth();
    p.synth.lengthSeconds = spring.lengthSeconds;
    p.synth.late = 0.0f;  // (the spring alone: no late field under it)
    p.spring = spring;
}

// A new entry of _pendingIrs with what every kind of IR has: its place, and the shape, EQ and damping that are set now
Convolution::PendingIr& Convolution::pend(size_t idx, size_t nframes) {
    _pendingIrs.emplace_back();
    PendingIr& p = _pendingIrs.back();
    p.idx = idx, p.nframes = nframes;
    p.shape = _irShape, p.eq = _irEq, p.damp = _irDamp;
    if (idx + 1 > _nirs) _nirs = idx + 1;
    return p;
}

void Convolution::prepareSynth(size_t idx, const IrSynth& synth, size_t nframes) {
    if (_group) {
        Log::error("conv", "IR synthesis is not available with several devices (mc_synth_ir is single-engine)");
        std::exit(2);
    }
    PendingIr& p = pend(idx, nframes);  // (generated by onStart(), once the client's rate is known)
    p.generated = true;
    p.synth = synth;
}

void Convolution::prepareSynth(size_t idx, const mc_ir_synth& synth, size_t nframes) {
    if (_group) {
        Log::error("conv", "IR synthesis is not available with several devices (mc_synth_ir is single-engine)");
        std::exit(2);
    }
    IrLoadRequest r = requestNow(idx, nframes, _irShape, _irEq, _irDamp);
    r.synth = synth;
    loadIr(r);
    if (idx + 1 > _nirs) _nirs = idx + 1;
}

mc_sweep Convolution::sweepFrames(const IrSweep& w, double rate) {
    const auto frames = [&](double seconds) { return std::nearbyint(seconds * rate); };
    mc_sweep s;
    mc_default_sweep(&s);
    s.rate = (uint32_t)rate;
    s.frames = (uint64_t)frames(w.lengthSeconds);
    s.f1_hz = w.f1;
    s.f2_hz = w.f2;
    s.amplitude = w.amp;
    s.fade_in = (uint32_t)std::min(frames(w.fadeInSeconds), 4294967295.0);
    s.fade_out = (uint32_t)std::min(frames(w.fadeOutSeconds), 4294967295.0);
    return s;
}

bool Convolution::writeSweep(const IrSweep& sweep, unsigned rate, std::string& why) {
    if (!mc_sweep_generate || !mc_default_sweep) {
        why = "the engine has no sweep (mc_sweep_generate)";
        return false;
    }
    const mc_sweep s = sweepFrames(sweep, (double)rate);
    std::vector<float> mono(s.frames <= (1ull << 22) ? s.frames : 0);
    if (mc_sweep_generate(&s, mono.data(), 0, s.frames) != MC_OK) {
        why = mc_last_error();
        return false;
    }
    std::vector<float> lr(2 * mono.size());
    for (size_t n = 0; n < mono.size(); n++) lr[2 * n] = lr[2 * n + 1] = mono[n];
    if (!WavFile::write(sweep.recording, lr.data(), mono.size(), 24, rate)) {
        why = "cannot write '" + sweep.recording + "'";
        return false;
    }
    return true;
}

void Convolution::prepareSweep(size_t idx, const IrSweep& sweep, const WavFile& recording, size_t nframes) {
    if (_group) {
        Log::error("conv", "sweep capture is not available with several devices (mc_load_ir_sweep is single-engine)");
        std::exit(2);
    }
    const float* lr = &recording.buffer[0].x;  // (deconvolved by onStart(), once the client's rate is known)
    PendingIr& p = pend(idx, nframes);
    p.rate = recording.sampleRate;
    p.lr.assign(lr, lr + 2 * recording.numFrames);
    p.swept = true;
    p.sweep = sweep;
}

Convolution::IrLoadRequest Convolution::requestNow(size_t idx, size_t nframes, const IrShape& shape, const IrEq& eq, const IrDamp& damp) const {
    IrLoadRequest r;
    r.idx = idx, r.nframes = nframes;
    r.shape = shape, r.eq = eq, r.damp = damp;
    r.phase = _irPhase.minimum ? &_irPhase : nullptr;
    r.filter = _irFilter.on ? &_irFilter : nullptr;
    r.match = _irMatch.on ? &_irMatch : nullptr;
    r.parts = _irParts.on ? &_irParts : nullptr;
    return r;
}

Convolution::IrLoadRequest Convolution::requestFor(const PendingIr& p) {
    IrLoadRequest r = requestNow(p.idx, p.nframes, p.shape, p.eq, p.damp);
    if (p.swept) {
        if (!mc_default_sweep) {
            Log::error("conv", "the engine has no sweep capture (mc_load_ir_sweep)");
            std::exit(2);
        }
        if (p.rate != samplerate) {
            Log::error("conv", "IR %zu: the recording '%s' is at %u Hz, the client at %zu Hz (a recorded sweep is not converted)", p.idx,
                       p.sweep.recording.c_str(), p.rate, (size_t)samplerate);
            std::exit(2);
        }
        SweepLoad w;
        w.sweep = sweepFrames(p.sweep, (double)samplerate);
        w.offset = (int64_t)std::nearbyint(p.sweep.offsetSeconds * (double)samplerate);
        const int64_t M = (int64_t)(p.lr.size() / 2), cap = 1ll << 24;
        int64_t F = p.sweep.irLengthSeconds > 0.0 ? (int64_t)std::nearbyint(p.sweep.irLengthSeconds * (double)samplerate)
                                                  : M - (int64_t)w.sweep.frames + 1 - w.offset;  // what the recording holds past the sweep
        if (!(p.sweep.irLengthSeconds > 0.0)) F = std::min(F, std::min(cap, (int64_t)((1ull << 40) / std::max<uint64_t>(w.sweep.frames, 1))));
        w.irFrames = (uint64_t)std::max<int64_t>(F, 1);
        r.lr = p.lr.data(), r.frames = (uint64_t)M;
        r.sweep = w;
        return r;
    }
    if (p.generated) {
        if (p.roomed && p.room.headed && !mc_default_ir_room_head) {
            Log::error("conv", "the engine has no binaural listener in its rooms (mc_synth_ir_room_head)");
            std::exit(2);
        }
        if (p.roomed && p.room.banded && !mc_default_ir_room_bands) {
            Log::error("conv", "the engine has no frequency bands in its rooms (mc_synth_ir_room_bands)");
            std::exit(2);
        }
        if (p.roomed && p.room.directional && !mc_default_ir_room_mics) {
            Log::error("conv", "the engine has no directional microphones in its rooms (mc_synth_ir_room_mics)");
            std::exit(2);
        }
        if (p.roomed && !mc_default_ir_room) {
            Log::error("conv", "the engine has no room rendering (mc_synth_ir_room)");
            std::exit(2);
        }
        if (p.plated && !mc_default_ir_plate) {
            Log::error("conv", "the engine has no plate synthesis (mc_synth_ir_plate)");
            std::exit(2);
        }
        if (p.sprung && !mc_default_ir_spring) {
            Log::error("conv", "the engine has no spring synthesis (mc_synth_ir_spring)");
            std::exit(2);
        }
        if (!mc_default_ir_synth) {
            Log::error("conv", "the engine has no IR synthesis (mc_synth_ir)");
            std::exit(2);
        }
        r.synth = synthFrames(p.roomed ? p.room.late : p.synth, (double)samplerate);
        if (p.plated) r.plate = plateFrames(p.plate, (double)samplerate);
        if (p.sprung) r.spring = springFrames(p.spring, (double)samplerate);
        if (p.roomed) r.room = roomFrames(p.room, (double)samplerate);
        if (p.roomed && p.room.directional) r.mics = roomMics(p.room);
        if (p.roomed && p.room.banded) r.bands = roomBands(p.room);
        if (p.roomed && p.room.headed) r.head = roomHead(p.room);
        return r;
    }
    r.lr = p.lr.data(), r.frames = p.lr.size() / 2;
    r.irRate = p.match && p.rate && p.rate != samplerate ? p.rate : 0;  // (0: loaded at the rate they have)
    r.sessionRate = (unsigned)samplerate;
    return r;
}

void Convolution::loadPendingIrs() {
    for (const PendingIr& p : _pendingIrs) {
        std::optional<mc_ir_tail> tail;
        std::optional<PartsSplit> split;
        if (_irTail.mode != IrTail::Off) tail = measureTail(p);
        if (_irParts.on && _irParts.splitAtMix) split = measureParts(p, tail);
        IrLoadRequest r = requestFor(p);
        r.tail = tail, r.split = split;
        loadIr(r);
        if (_rt60 > 0.0) aimRt60(r);
        if (_decayReport) reportDecay(p.idx);
        if (_floorReport) reportFloor(p.idx);
        if (_densityReport) reportDensity(p.idx);
        if (_iaccReport) reportIacc(p.idx);
        if (_stiReport) reportSti(p.idx);
        if (_responseReport) reportResponse(p.idx);
    }
    _pendingIrs.clear();
}

void Convolution::prepare(size_t idx, const WavFile& wav, size_t nframes) {
    if (_matchIrRate || !_irEq.off() || !_irDamp.off() || _decayReport || _rt60 > 0.0 || _floorReport || _densityReport || _iaccReport || _stiReport || _responseReport || _irTail.mode != IrTail::Off || _irPhase.minimum || _irFilter.on || _irMatch.on || _irParts.on) {  // (loaded by onStart(), once the client's rate is known)
        const float* lr = &wav.buffer[0].x;
        PendingIr& p = pend(idx, nframes);
        p.rate = wav.sampleRate;
        p.lr.assign(lr, lr + 2 * wav.numFrames);
        p.match = _matchIrRate;
        return;
    }
    if (!_irShape.off()) {  // (never with several devices: setIrShape)
        IrLoadRequest r = requestNow(idx, nframes, _irShape, IrEq(), IrDamp());  // (no rates: the frames are loaded at the rate they have)
        r.lr = &wav.buffer[0].x, r.frames = wav.numFrames;
        loadIr(r);
        if (idx + 1 > _nirs) _nirs = idx + 1;
        return;
    }
    if (_group) {
        if (mc_group_load_ir(_group, idx, &wav.buffer[0].x, wav.numFrames, nframes) != MC_OK) {
            Log::error("conv", "mc_group_load_ir failed: %s", mc_group_last_error());
            std::abort();
        }
    } else
        check(mc_load_ir(_engine, idx, &wav.buffer[0].x, wav.numFrames, nframes), "mc_load_ir");
    if (idx + 1 > _nirs) _nirs = idx + 1;
}

// cc[i].value is plain public data written by main() and by the MIDI thread
// (main.cu:49-70, conv.cu:255-276); it is handed to the engine at each block.
void Convolution::pushParams() {
    for (int i = 0; i < 2; i++) {
        mc_cc_value v;
        v.select = cc[i].value.select;
        v.predelay = cc[i].value.predelay;
        v.speed = cc[i].value.speed;
        v.vsteps = _pushedVsteps[i] = cc[i].value.vsteps;
        v.dry = cc[i].value.dry;
        v.wet = cc[i].value.wet;
        v.panDry = cc[i].value.panDry;
        v.panWet = cc[i].value.panWet;
        v.level = cc[i].value.level;
        if (_group) {
            if (mc_group_set_params(_group, i, &v) != MC_OK) {
                Log::error("conv", "mc_group_set_params failed: %s", mc_group_last_error());
                std::abort();
            }
        } else
            check(mc_set_params(_engine, i, &v), "mc_set_params");
    }
}

void Convolution::pullVsteps() {
    for (int i = 0; i < 2; i++) {
        mc_cc_value v;
        check(mc_get_params(_engine, i, &v), "mc_get_params");
        // counts down once per block (conv.cu:345,353).  A select that arrived from the MIDI thread while the engine
        // was processing has reset vsteps to speed (conv.cu:261): like the reference's in-place decrement, the
        // write-back must not undo it - only the value that was handed to the engine is replaced
        if (cc[i].value.vsteps == _pushedVsteps[i]) cc[i].value.vsteps = v.vsteps;
    }
}

void Convolution::onProcess(size_t nframes) {
    auto in1 = capture[0] ? (const float*)jack_port_get_buffer(capture[0], nframes) : nullptr;
    auto in2 = capture[1] ? (const float*)jack_port_get_buffer(capture[1], nframes) : nullptr;
    auto L = playback[0] ? (float*)jack_port_get_buffer(playback[0], nframes) : nullptr;
    auto R = playback[1] ? (float*)jack_port_get_buffer(playback[1], nframes) : nullptr;
    if (!in1 || !in2 || !L || !R) return;  // conv.cu:297
    if (_group) {
        Log::error("conv", "a Convolution over several devices renders batches only (processBatch)");
        std::abort();
    }
    if (nframes != _period) {  // jackd decides the period (256 on the README's target, 512 / 1024 in the run scripts)
        check(mc_set_period(_engine, (uint32_t)nframes), "mc_set_period");
        _period = nframes;
    }
    pushParams();
    check(mc_process(_engine, in1, in2, L, R, nframes), "mc_process");
    pullVsteps();
}

void Convolution::processBatch(const float* in1, const float* in2, float* outL, float* outR, size_t nblocks) {
    pushParams();
    for (size_t done = 0; done < nblocks;) {
        const size_t n = nblocks - done < _maxBatch ? nblocks - done : _maxBatch;
        if (_group) {
            if (mc_group_process_batch(_group, in1 + done * 256, in2 + done * 256, outL + done * 256, outR + done * 256, n) != MC_OK) {
                Log::error("conv", "mc_group_process_batch failed: %s", mc_group_last_error());
                std::abort();
            }
        } else
            check(mc_process_batch(_engine, in1 + done * 256, in2 + done * 256, outL + done * 256, outR + done * 256, n),
                  "mc_process_batch");
        done += n;
        pullVsteps();
        pushParams();
    }
}

double Convolution::avgRuntime() const { return mc_avg_runtime_ms(_engine); }

void Convolution::onMidiMessage(const RawMidi::Device* sender, const uint8_t* buffer, size_t len) {
    // conv.cu:278-285 + handleCC :255-276, applied to the public cc[] values
    if (len < 3) return;
    for (int i = 0; i < 2; i++) {
        CC& c = cc[i];
        if (c.device != sender || c.message != buffer[0]) continue;
        const uint8_t m2 = buffer[1];
        const int v = buffer[2];
        if (c.select == m2) {
            c.value.select = (size_t)v * _nirs / 0x80;
            c.value.vsteps = c.value.speed;
            Log::info("conv", "Selected IR %zu", c.value.select);
        }
        if (c.predelay == m2) c.value.predelay = (size_t)v * CONV_MAX_PREDELAY / 0x80;
        if (c.dry == m2) c.value.dry = v / 128.0f;
        if (c.wet == m2) c.value.wet = v / 128.0f;
        if (c.panDry == m2) c.value.panDry = v / 64.0f - 1;
        if (c.panWet == m2) c.value.panWet = v / 64.0f - 1;
        if (c.level == m2) c.value.level = v / 128.0f;
        if (c.speed == m2) {
            c.value.speed = ((size_t)v * CONV_MAX_SPEED) / 0x80;
            if (c.value.vsteps > c.value.speed) c.value.vsteps = c.value.speed;
        }
    }
}
