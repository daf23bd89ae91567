// main.cpp — application wiring in the order of the reference's main()
// (src/main.cu:18-116): select GPU, read settings.txt, one Convolution per
// pair of channels, per half the MIDI mapping + initial values + IR bank,
// start, connect ports, wait for a key, report the average runtime.
// Built against the fake JACK of this directory it runs offline:
// `mcconv_host --periods N` drives N periods of synthetic input instead of
// waiting on stdin - all instances AT ONCE, a driver thread per client, as jackd
// runs them (--sequential: one after the other; --period F: frames per period;
// --spacing US: a period clock; --dump PREFIX: every instance's input and output
// as raw float32 files PREFIX<i>.in1 / .in2 / .outL / .outR; --rate HZ: the fake server's sample rate, 44100 unless
// given; --match-ir-rate: every IR is converted to the client's sample rate on load, Convolution::setMatchIrRate;
// --ir-start N, --ir-trim DB[:PREROLL], --ir-length N, --ir-reverse, --ir-decay N, --ir-fade N,
// --ir-normalize peak|energy[:TARGET]: every IR is shaped on load, Convolution::setIrShape - lengths in frames at the rate
// the IR is loaded at; --ir-eq KIND:HZ[:DB][:Q], up to 8 times, KIND one of lowcut, highcut, lowshelf, highshelf, peak (the cuts:
// KIND:HZ[:Q]): every IR is equalised on load with these bands in this order, at the client's sample rate,
// Convolution::setIrEq; --ir-decay-report: after each IR is loaded one log line with its decay (origin, EDT, T20, T30, C50, C80, Ts
// of the broadband LR row, measured by the engine: Convolution::setIrDecayReport), --ir-decay-bands HZ[,HZ...]: one more line per
// centre frequency; --ir-rt60 SECONDS: every IR whose measured decay time is longer is loaded again with the further exponential
// decay that takes it there, on top of --ir-decay, Convolution::setIrRt60; --ir-damp HZ[,HZ[,HZ]]:SEC[,SEC...]: every IR is damped on
// load, 1 to 3 ascending crossover frequencies and one further decay time in seconds per band, low to high, 0 for none, turned into
// frames at the client's sample rate, Convolution::setIrDamp; --ir-damp-origin TAP: the stored tap the damping's envelopes start at).
// A line of an IR index that starts with "synth:" is an IR the engine generates instead of a WAV path,
// synth:LENGTH_S:T60_S[:key=value,...] with keys seed, start, buildup, late, direct, early, efirst, elast, egain, width
// (Convolution::parseSynth; times in seconds at the client's sample rate); the --ir-* options apply to it as to a WAV.
// A line that starts with "room:" is a rectangular room whose reflections the engine renders (the image-source method),
// room:LENGTH_S:LX,LY,LZ:SX,SY,SZ:RX,RY,RZ[:key=value,...] with keys beta (one value, or six separated by '/'), order, spacing,
// axis (x|y|z), speed, gain, last (seconds), and t60 and synth:'s keys for a late field under it (Convolution::parseRoom; metres and
// seconds); the --ir-* options apply to it as to a WAV, --ir-tail included: a short rendering runs out at its own measured slope.
// Directional microphones and a directional source in that room: mic=P or mic=P/P (left/right; P one of omni, subcardioid,
// cardioid, supercardioid, hypercardioid, fig8, or alpha in [0, 1]), aim=AZ or AZ/AZ and tilt=EL or EL/EL in degrees (azimuth
// from +x towards +y, tilt towards +z), src=P, srcaim=AZ, srctilt=EL; one more log line tells the direct sound's factors.
// Walls and air per frequency band in that room: xover=HZ[/HZ[/HZ]] cuts up to four bands, betas=B[/B...] gives every band one
// reflection coefficient for its six walls, air=DB[/DB...] the air's loss in dB per metre (one value, or one per band); the room
// is rendered once per band and joined by --ir-damp's band split, and one more log line tells the bands' reverberation times.
// A line that starts with "plate:" is a plate reverberator whose modes the engine sums, plate:LENGTH_S[:key=value,...] with keys
// size=LX,LY, thick=MM, material=steel|E/RHO/NU, drive=X,Y, pick=X,Y/X,Y, low=HZ, high=HZ, t60=LO/HI, damp=HZ, gain, last=S
// (Convolution::parsePlate; metres, millimetres and seconds); the --ir-* options apply to it as to a WAV, and one more log line
// tells the modes kept.
// A line that starts with "spring:" is a spring reverberation tank whose response the engine evaluates bin by bin,
// spring:LENGTH_S[:key=value,...] with keys sections, fc=HZ, a, delay=MS[,MS[,MS]], t60=S, damping, lowpass=ORDER, high, highsections,
// higha, highdelay, hight60=S, stereo, gain, points, last=S (Convolution::parseSpring; Hz, milliseconds and seconds); the --ir-*
// options apply to it as to a WAV, and one more log line tells the transform's size, the delays and the alias bound.
// A line that starts with "sweep:" is an IR the engine deconvolves from the recording of a sine sweep,
// sweep:RECORDING.wav:LENGTH_S:F1:F2[:key=value,...] with keys amp, fadein, fadeout, offset, length (Convolution::parseSweep;
// times in seconds, the recording at the client's sample rate); the --ir-* options apply to it as to a WAV.
// --write-sweep FILE.wav:LENGTH_S:F1:F2[:key=value,...] writes that sweep (keys amp, fadein, fadeout) at --rate (44100 without)
// to both channels of a 24-bit WAV file and exits: what to play through the room.
// --ir-floor-report: after each IR is loaded one log line per row group with its noise floor (knee, late decay time, noise level,
// peak to noise, measured by the engine: Convolution::setIrFloorReport); --ir-floor-xovers HZ[,HZ[,HZ]]: the crossovers whose bands
// are row groups of their own, and the bands of --ir-tail; --ir-tail cut|extend[:fade=S,length=S,seed=N,width=W]: every IR is
// loaded, its floor measured, and loaded again with every band cut at its knee or extended from there with decaying noise,
// ahead of the other --ir-* options, Convolution::setIrTail; an IR with less than 30 dB between peak and floor is left as it is.
// --ir-phase minimum[:floor=DB,over=K]: every IR (a WAV or a captured sweep; a generated one is left as it is) is converted to
// minimum phase on load, after --ir-tail's step and ahead of the other --ir-* options: the same magnitude response with the
// delay inside the IR taken out (Convolution::setIrPhase; floor: the dynamic range of the log spectrum in dB, 120 without; over:
// the oversampling of the transform, 2 .. 64, 8 without); one log line tells the delay removed and what the truncation kept.
// --ir-filter FILE.wav[:op=deconvolve,channels=mid,reg=DB,keep=SECONDS]: every IR (a WAV or a captured sweep; a generated one is
// left as it is) is convolved on load with the stereo IR in FILE.wav, converted from that file's rate to the client's, after
// --ir-phase's step and ahead of the other --ir-* options, so that the cascade of the two runs as one IR
// (Convolution::setIrFilter); op=deconvolve divides FILE.wav out of the IR instead, reg dB (60 without) below its strongest bin;
// channels: stereo (without), left, or mid = (L + R) / 2 for both; keep: the seconds the step hands on (all of a convolution, the
// IR's own length of a deconvolution without); one log line tells the lengths and the level.
// --ir-match FILE.wav|flat[:amount=A,boost=DB,cut=DB,smooth=OCTAVES,lo=HZ,hi=HZ,link=0,phase=linear,delay=SECONDS,tilt=DB]: every IR (a
// WAV or a captured sweep; a generated one is left as it is) gets on load the tonal balance of the stereo IR in FILE.wav, converted
// from that file's rate to the client's, or with `flat` of a line that tilts by tilt dB per octave (0 whitens, -3 aims at pink),
// after --ir-filter's step and ahead of the other --ir-* options (Convolution::setIrMatch): the third-octave-smoothed (smooth)
// spectra are compared from lo to hi Hz (20 Hz to 20 kHz or half the rate without), amount (1 without) of the difference, less
// its mean, is bounded to boost and cut dB (12 and 24 without) and applied as a minimum-phase correction, or with phase=linear
// as a linear-phase one that delays the IR by delay seconds; link=0 gives each channel a curve of its own; one log line tells the
// lengths, the curve's range and the level.  --ir-match-report: one more line per grid point with the curve.
// --ir-parts direct=DB|off,early=DB|off,late=DB|off[,split=SECONDS|mix,first=SECONDS,onset=SECONDS,xfade=S:S,delay=S:S:S,width=W[:W:W],
// balance=B[:B:B],swap[=PARTS],invert[=PARTS]]: every IR (a WAV or a captured sweep; a generated one is left as it is) is split on
// load into its direct sound, its early reflections and its late tail, after --ir-match's step and ahead of the other --ir-*
// options (Convolution::setIrParts): each part gets a gain in dB or is taken out (off), a delay in seconds (negative: earlier), a
// width (0 mono, 1 as it is, 2 the side signal doubled) and a balance (-1 left .. +1 right); the direct part ends `first` seconds
// (2.5 ms without) and the early part `split` seconds (80 ms without) after `onset` (0 without), with cross-fades of xfade
// seconds around the two; split=mix: the IR is loaded once without the step, and the onset and the early part's end are the
// origin and the mixing tap of its echo density (--ir-density-window and -hop apply); swap exchanges and invert negates the
// channels of the named parts (direct:early:late; all without names); one log line tells the boundaries, the energies and what
// was lost.
// --ir-density-report: after each IR is loaded one log line with its echo density (origin, mixing tap and time, first, largest and
// later density of the LR row, measured by the engine: Convolution::setIrDensityReport); --ir-density-window SECONDS: the whole
// window (20 ms without), --ir-density-hop SECONDS: between window centres (an eighth of the window without), --ir-density-t60
// SECONDS|auto: the decay undone inside each window, auto: the measured T30.  --ir-tail's key knee=floor|mix: with mix (extend
// only) the knees the floor search placed are moved to that mixing tap, which is where a rendered room hands over to its tail.
// --ir-iacc-report: after each IR is loaded one log line per window (early, late, all) with its interaural cross-correlation
// (origin, IACC, its lag in taps and ms, IACF(0), level difference, status; measured by the engine: Convolution::setIrIaccReport);
// --ir-iacc-bands HZ[,HZ...]: one more line per band for the whole IR; --ir-iacc-lag SECONDS: the largest lag (1 ms without).
// --ir-tail's key width=iacc (extend only): the tail's width is 1 - the late broadband IACF(0) measured on the same load.
// --ir-sti-report: after each IR is loaded one log line per channel set (L, R, LR) with its speech transmission index (origin,
// STI and its rating, the seven octaves' MTI, status; measured by the engine: Convolution::setIrStiReport); --ir-sti-snr
// DB[,DB...]: stationary noise at that signal-to-noise ratio, one value for all octaves or one per octave.
// --ir-response-report: after each IR is loaded one log line per channel with its frequency response (origin, the level at
// 1 kHz, the octaves 31.5 Hz .. 16 kHz relative to it, the group delay at 1 kHz, status; measured by the engine:
// Convolution::setIrResponseReport); --ir-response-smooth OCTAVES: the width the levels are smoothed over (1 without).
#include <cassert>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <random>
#include <vector>

#include "conv.h"
#include "settings.h"

// text through one of Convolution's argument parsers into out; false, with "<what> '<text>': <the parser's reason>" on stderr, for
// a text the parser refuses (what: the option, or "index line")
template <typename T>
static bool parsed(const char* what, const std::string& text, T& out, bool (*parse)(const std::string&, T&, std::string&)) {
    std::string why;
    if (parse(text, out, why)) return true;
    std::cerr << what << " '" << text << "': " << why << std::endl;
    return false;
}
// (the parsers of several options take the option first)
template <typename T>
static bool parsed(const char* option, const std::string& text, T& out, bool (*parse)(const std::string&, const std::string&, T&, std::string&)) {
    std::string why;
    if (parse(option, text, out, why)) return true;
    std::cerr << option << " '" << text << "': " << why << std::endl;
    return false;
}

int main(int argc, char** argv) {
    uint64_t periods = 0;
    const char* settingsPath = "settings.txt";
    const char* dump = nullptr;
    bool sequential = false;
    double spacing_us = 0.0;
    jack_nframes_t rate = 0, period = 0;  // fake JACK server: 0 = its defaults (44100 Hz, 256 frames)
    bool matchIrRate = false;
    Convolution::IrShape irShape;
    Convolution::IrEq irEq;
    bool irDecayReport = false;
    std::vector<float> irDecayBands;
    double irRt60 = 0.0;
    Convolution::IrDamp irDamp;
    const char* writeSweep = nullptr;
    bool irFloorReport = false;
    std::vector<float> irFloorXovers;
    Convolution::IrTail irTail;
    Convolution::IrPhase irPhase;
    Convolution::IrFilter irFilter;
    Convolution::IrMatch irMatch;
    Convolution::IrParts irParts;
    bool irMatchReport = false;
    bool irDensityReport = false;
    Convolution::DensityQuery irDensity;
    bool irIaccReport = false;
    Convolution::IaccQuery irIacc;
    bool irStiReport = false;
    Convolution::StiQuery irSti;
    bool irResponseReport = false;
    Convolution::ResponseQuery irResponse;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--periods") && i + 1 < argc) periods = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "--settings") && i + 1 < argc) settingsPath = argv[++i];
        else if (!strcmp(argv[i], "--dump") && i + 1 < argc) dump = argv[++i];
        else if (!strcmp(argv[i], "--sequential")) sequential = true;
        else if (!strcmp(argv[i], "--spacing") && i + 1 < argc) spacing_us = atof(argv[++i]);
        else if (!strcmp(argv[i], "--period") && i + 1 < argc) period = (jack_nframes_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "--rate") && i + 1 < argc) rate = (jack_nframes_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "--write-sweep") && i + 1 < argc) writeSweep = argv[++i];
        else if (!strcmp(argv[i], "--match-ir-rate")) matchIrRate = true;
        else if (!strcmp(argv[i], "--ir-start") && i + 1 < argc) irShape.start = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "--ir-trim") && i + 1 < argc) {
            char* end = nullptr;
            irShape.trimDb = strtof(argv[++i], &end);
            if (*end == ':') irShape.preRoll = (uint32_t)strtoul(end + 1, nullptr, 10);
        } else if (!strcmp(argv[i], "--ir-length") && i + 1 < argc) irShape.length = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "--ir-reverse")) irShape.reverse = true;
        else if (!strcmp(argv[i], "--ir-decay") && i + 1 < argc) irShape.decayT60 = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "--ir-fade") && i + 1 < argc) irShape.fadeOut = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "--ir-normalize") && i + 1 < argc) {
            const char* a = argv[++i];
            const char* colon = strchr(a, ':');
            const size_t len = colon ? (size_t)(colon - a) : strlen(a);
            if (len == 4 && !strncmp(a, "peak", 4)) irShape.normalize = Convolution::IrShape::Peak;
            else if (len == 6 && !strncmp(a, "energy", 6)) irShape.normalize = Convolution::IrShape::Energy;
            else {
                std::cerr << "--ir-normalize takes peak or energy, optionally :TARGET" << std::endl;
                return 2;
            }
            if (colon) irShape.target = strtof(colon + 1, nullptr);
        } else if (!strcmp(argv[i], "--ir-eq") && i + 1 < argc) {
            using Band = Convolution::IrEq::Band;
            static const struct { const char* name; Band::Kind kind; } kinds[] = {
                {"lowcut", Band::LowCut}, {"highcut", Band::HighCut}, {"lowshelf", Band::LowShelf}, {"highshelf", Band::HighShelf}, {"peak", Band::Peak}};
            const char* a = argv[++i];
            const char* colon = strchr(a, ':');
            Band b;
            for (auto& k : kinds)
                if (colon && strlen(k.name) == (size_t)(colon - a) && !strncmp(a, k.name, colon - a)) b.kind = k.kind;
            if (b.kind == Band::Off || irEq.bands.size() == 8) {
                std::cerr << "--ir-eq takes lowcut|highcut:HZ[:Q] or lowshelf|highshelf|peak:HZ[:DB][:Q], at most 8 times" << std::endl;
                return 2;
            }
            char* end = nullptr;
            b.hz = strtof(colon + 1, &end);
            const bool cut = b.kind == Band::LowCut || b.kind == Band::HighCut;
            if (*end == ':' && !cut) b.gainDb = strtof(end + 1, &end);
            if (*end == ':') b.q = strtof(end + 1, &end);
            irEq.bands.push_back(b);
        } else if (!strcmp(argv[i], "--ir-decay-report")) irDecayReport = true;
        else if (!strcmp(argv[i], "--ir-decay-bands") && i + 1 < argc) {
            irDecayReport = true;
            for (const char* a = argv[++i]; *a;) {
                char* end = nullptr;
                irDecayBands.push_back(strtof(a, &end));
                if (end == a || (*end && *end != ',') || irDecayBands.size() > 10) {
                    std::cerr << "--ir-decay-bands takes HZ[,HZ...], at most 10" << std::endl;
                    return 2;
                }
                a = *end ? end + 1 : end;
            }
        } else if (!strcmp(argv[i], "--ir-damp") && i + 1 < argc) {
            const char* a = argv[++i];
            const char* colon = strchr(a, ':');
            bool good = colon != nullptr;
            irDamp.xovers.clear();
            irDamp.decaySeconds.clear();
            for (int part = 0; part < 2 && good; part++) {  // HZ[,HZ[,HZ]] up to the colon, then SEC[,SEC...]
                const char* stop = part ? a + strlen(a) : colon;
                for (const char* p = part ? colon + 1 : a; good;) {
                    char* end = nullptr;
                    const double v = strtod(p, &end);
                    good = end != p && end <= stop && (end == stop || *end == ',') && v >= 0.0 && v < 1e9;
                    if (!good) break;
                    if (part) irDamp.decaySeconds.push_back(v);
                    else irDamp.xovers.push_back((float)v);
                    if (end == stop) break;
                    p = end + 1;
                }
            }
            if (!good || irDamp.xovers.empty() || irDamp.xovers.size() > 3 || irDamp.decaySeconds.size() != irDamp.xovers.size() + 1) {
                std::cerr << "--ir-damp takes HZ[,HZ[,HZ]]:SEC[,SEC...]: 1 to 3 crossovers and one decay time in seconds per band (one more than crossovers), 0 for none"
                          << std::endl;
                return 2;
            }
        } else if (!strcmp(argv[i], "--ir-damp-origin") && i + 1 < argc) {
            char* end = nullptr;
            const char* a = argv[++i];
            irDamp.origin = strtoull(a, &end, 10);
            if (end == a || *end || *a == '-') {
                std::cerr << "--ir-damp-origin takes a tap index" << std::endl;
                return 2;
            }
        } else if (!strcmp(argv[i], "--ir-floor-report")) irFloorReport = true;
        else if (!strcmp(argv[i], "--ir-floor-xovers") && i + 1 < argc) {
            irFloorXovers.clear();
            for (const char* a = argv[++i];;) {
                char* end = nullptr;
                irFloorXovers.push_back(strtof(a, &end));
                if (end == a || (*end && *end != ',') || irFloorXovers.size() > 3 || !(irFloorXovers.back() > 0.f) ||
                    (irFloorXovers.size() > 1 && !(irFloorXovers.back() > irFloorXovers[irFloorXovers.size() - 2]))) {
                    std::cerr << "--ir-floor-xovers takes HZ[,HZ[,HZ]]: 1 to 3 ascending crossover frequencies" << std::endl;
                    return 2;
                }
                if (!*end) break;
                a = end + 1;
            }
        } else if (!strcmp(argv[i], "--ir-tail") && i + 1 < argc) {
            if (!parsed("--ir-tail", argv[++i], irTail, Convolution::parseTail)) return 2;
        } else if (!strcmp(argv[i], "--ir-phase") && i + 1 < argc) {
            if (!parsed("--ir-phase", argv[++i], irPhase, Convolution::parsePhase)) return 2;
        } else if (!strcmp(argv[i], "--ir-filter") && i + 1 < argc) {
            if (!parsed("--ir-filter", argv[++i], irFilter, Convolution::parseFilter)) return 2;
            if (!std::ifstream(irFilter.path, std::ifstream::binary).good()) {
                std::cerr << "--ir-filter '" << argv[i] << "': cannot open " << irFilter.path << std::endl;
                return 2;
            }
            const WavFile wav(irFilter.path);
            irFilter.rate = wav.sampleRate;
            irFilter.lr.assign(&wav.buffer[0].x, &wav.buffer[0].x + 2 * wav.numFrames);
        } else if (!strcmp(argv[i], "--ir-match") && i + 1 < argc) {
            if (!parsed("--ir-match", argv[++i], irMatch, Convolution::parseMatch)) return 2;
            if (!irMatch.flat) {
                if (!std::ifstream(irMatch.path, std::ifstream::binary).good()) {
                    std::cerr << "--ir-match '" << argv[i] << "': cannot open " << irMatch.path << std::endl;
                    return 2;
                }
                const WavFile wav(irMatch.path);
                irMatch.rate = wav.sampleRate;
                irMatch.lr.assign(&wav.buffer[0].x, &wav.buffer[0].x + 2 * wav.numFrames);
            }
        } else if (!strcmp(argv[i], "--ir-parts") && i + 1 < argc) {
            if (!parsed("--ir-parts", argv[++i], irParts, Convolution::parseParts)) return 2;
        } else if (!strcmp(argv[i], "--ir-match-report")) irMatchReport = true;
        else if (!strcmp(argv[i], "--ir-density-report")) irDensityReport = true;
        else if ((!strcmp(argv[i], "--ir-density-window") || !strcmp(argv[i], "--ir-density-hop") || !strcmp(argv[i], "--ir-density-t60")) && i + 1 < argc) {
            const char* option = argv[i];
            if (!parsed(option, argv[++i], irDensity, Convolution::parseDensity)) return 2;
        } else if (!strcmp(argv[i], "--ir-iacc-report")) irIaccReport = true;
        else if ((!strcmp(argv[i], "--ir-iacc-lag") || !strcmp(argv[i], "--ir-iacc-bands")) && i + 1 < argc) {
            const char* option = argv[i];
            if (!parsed(option, argv[++i], irIacc, Convolution::parseIacc)) return 2;
        } else if (!strcmp(argv[i], "--ir-sti-report")) irStiReport = true;
        else if (!strcmp(argv[i], "--ir-sti-snr") && i + 1 < argc) {
            if (!parsed("--ir-sti-snr", argv[++i], irSti, Convolution::parseSti)) return 2;
        } else if (!strcmp(argv[i], "--ir-response-report")) irResponseReport = true;
        else if (!strcmp(argv[i], "--ir-response-smooth") && i + 1 < argc) {
            if (!parsed("--ir-response-smooth", argv[++i], irResponse, Convolution::parseResponse)) return 2;
        } else if (!strcmp(argv[i], "--ir-rt60") && i + 1 < argc) {
            irRt60 = atof(argv[++i]);
            if (!(irRt60 > 0.0)) {
                std::cerr << "--ir-rt60 takes a decay time in seconds, > 0" << std::endl;
                return 2;
            }
        }
    }
    if (writeSweep) {  // (before any device is looked at: host arithmetic only)
        Convolution::IrSweep sweep;
        std::string why;
        if (!Convolution::parseSweep(std::string("sweep:") + writeSweep, sweep, why) || !Convolution::writeSweep(sweep, rate ? rate : 44100, why)) {
            std::cerr << "--write-sweep '" << writeSweep << "': " << why << std::endl;
            return 2;
        }
        std::cout << "wrote " << sweep.recording << std::endl;
        return 0;
    }
    if (rate || period) fakejack_configure(rate ? rate : 44100, period ? period : 256);
    selectGpu();

    Settings settings;
    settings.open(settingsPath);
    auto count = settings.u32("conv.count");
    assert(count % 2 == 0 && "conv.count must be a multiple of 2");
    count /= 2;

    std::map<std::string, RawMidi::Device*> midiDevices;
    std::vector<Convolution*> instances;
    for (uint32_t n = 0; n < count; n++) {
        const auto fs1 = settings.u32("conv[%d].fftSize", n * 2 + 0);
        const auto fs2 = settings.u32("conv[%d].fftSize", n * 2 + 1);
        assert(fs1 == fs2 && "a convolution pair needs identical fft sizes");
        auto* c = new Convolution(std::string("hipconv_") + char('1' + n), fs1);
        instances.push_back(c);
        if (matchIrRate) c->setMatchIrRate(true);
        c->setIrShape(irShape);
        c->setIrEq(irEq);
        c->setIrDamp(irDamp);
        if (irDecayReport) c->setIrDecayReport(true, irDecayBands);
        if (irRt60 > 0.0) c->setIrRt60(irRt60);
        c->setIrFloorXovers(irFloorXovers);
        if (irFloorReport) c->setIrFloorReport(true);
        c->setIrDensityReport(irDensityReport, irDensity);
        c->setIrIaccReport(irIaccReport, irIacc);
        c->setIrStiReport(irStiReport, irSti);
        c->setIrResponseReport(irResponseReport, irResponse);
        c->setIrTail(irTail);
        c->setIrPhase(irPhase);
        c->setIrFilter(irFilter);
        c->setIrMatch(irMatch, irMatchReport);
        c->setIrParts(irParts);
        for (int i = 0; i < 2; i++) {
            const int idx = n * 2 + i;
            const auto deviceId = settings.str("conv[%d].cc.device", idx);
            if (!deviceId.empty()) {
                auto& dev = midiDevices[deviceId];
                if (!dev) dev = new RawMidi::Device(deviceId);
                c->cc[i].device = dev;
                dev->handler = c;
            }
            // MIDI controller numbers and initial values, table-driven: "conv[<idx>].cc.<name>" / ".value.<name>"
            Convolution::CC& half = c->cc[i];
            struct { const char* name; uint8_t* slot; } controllers[] = {
                {"message", &half.message}, {"select", &half.select},   {"predelay", &half.predelay},
                {"dry", &half.dry},         {"wet", &half.wet},         {"speed", &half.speed},
                {"panDry", &half.panDry},   {"panWet", &half.panWet},   {"level", &half.level}};
            for (auto& k : controllers) *k.slot = settings.u8("conv[%d].cc.%s", idx, k.name);
            struct { const char* name; size_t* slot; } counts[] = {
                {"select", &half.value.select}, {"predelay", &half.value.predelay}, {"speed", &half.value.speed}};
            for (auto& k : counts) *k.slot = settings.u32("conv[%d].value.%s", idx, k.name);
            struct { const char* name; float* slot; } gains[] = {{"dry", &half.value.dry},
                                                                  {"wet", &half.value.wet},
                                                                  {"panDry", &half.value.panDry},
                                                                  {"panWet", &half.value.panWet},
                                                                  {"level", &half.value.level}};
            for (auto& k : gains) *k.slot = settings.f32("conv[%d].value.%s", idx, k.name);

            std::ifstream index(settings.str("conv[%d].index", idx));
            std::string path;
            for (size_t j = 0; std::getline(index, path); j++) {
                if (path.empty()) continue;
                if (!path.compare(0, 6, "synth:")) {  // a generated IR instead of a WAV path
                    Convolution::IrSynth synth;
                    if (!parsed("index line", path, synth, Convolution::parseSynth)) return 2;
                    c->prepareSynth(j, synth);
                    continue;
                }
                if (!path.compare(0, 5, "room:")) {  // a rendered room instead of a WAV path
                    Convolution::IrRoom room;
                    if (!parsed("index line", path, room, Convolution::parseRoom)) return 2;
                    c->prepareRoom(j, room);
                    continue;
                }
                if (!path.compare(0, 6, "plate:")) {  // a plate reverberator instead of a WAV path
                    Convolution::IrPlate plate;
                    if (!parsed("index line", path, plate, Convolution::parsePlate)) return 2;
                    c->preparePlate(j, plate);
                    continue;
                }
                if (!path.compare(0, 7, "spring:")) {  // a spring tank instead of a WAV path
                    Convolution::IrSpring spring;
                    if (!parsed("index line", path, spring, Convolution::parseSpring)) return 2;
                    c->prepareSpring(j, spring);
                    continue;
                }
                if (!path.compare(0, 6, "sweep:")) {  // an IR deconvolved from a recorded sweep
                    Convolution::IrSweep sweep;
                    if (!parsed("index line", path, sweep, Convolution::parseSweep)) return 2;
                    WavFile rec(sweep.recording);
                    c->prepareSweep(j, sweep, rec);
                    continue;
                }
                WavFile w(path);
                c->prepare(j, w);
            }
        }
        c->start();
        for (int i = 0; i < 2; i++) {
            const int idx = n * 2 + i;
            jack_connect(c->handle, settings.str("conv[%d].input", idx).c_str(), jack_port_name(c->capture[i]));
            jack_connect(c->handle, jack_port_name(c->playback[i]), settings.str("conv[%d].output", idx).c_str());
            if (auto* d = c->cc[i].device)
                if (!d->isOpen) d->start();
        }
    }

    if (periods) {
        // offline: the fake JACK server pushes seeded noise through every instance (its own stream of noise each), all
        // instances at once unless --sequential
        struct Feed {
            std::mt19937 rng;
            std::uniform_real_distribution<float> u{-0.25f, 0.25f};
            std::vector<float> rec[4];  // in1, in2, outL, outR when dumping
            bool keep = false;
        };
        std::vector<Feed> feeds(instances.size());
        std::vector<void*> users;
        std::vector<jack_client_t*> clients;
        for (size_t i = 0; i < instances.size(); i++) {
            feeds[i].rng.seed(1234 + 17 * (unsigned)i);
            feeds[i].keep = dump != nullptr;
            users.push_back(&feeds[i]);
            clients.push_back(instances[i]->handle);
        }
        auto fill = [](uint64_t, float** bufs, size_t n, jack_nframes_t nframes, void* user) {
            auto* f = static_cast<Feed*>(user);
            for (size_t b = 0; b < n; b++)
                for (jack_nframes_t s = 0; s < nframes; s++) {
                    bufs[b][s] = f->u(f->rng) + 0.01f;
                    if (f->keep && b < 2) f->rec[b].push_back(bufs[b][s]);
                }
        };
        auto keep = [](uint64_t, float** bufs, size_t n, jack_nframes_t nframes, void* user) {
            auto* f = static_cast<Feed*>(user);
            if (!f->keep) return;
            for (size_t b = 0; b < n && b < 2; b++) f->rec[2 + b].insert(f->rec[2 + b].end(), bufs[b], bufs[b] + nframes);
        };
        std::vector<double> us(instances.size(), 0.0);
        if (sequential)
            for (size_t i = 0; i < instances.size(); i++) fakejack_run_all(&clients[i], 1, periods, fill, keep, &users[i], spacing_us, &us[i]);
        else
            fakejack_run_all(clients.data(), clients.size(), periods, fill, keep, users.data(), spacing_us, us.data());
        for (size_t i = 0; i < instances.size(); i++) {
            Log::info(instances[i]->name, "%s: %.2f us per period inside the process callback (%llu periods)", sequential ? "alone" : "concurrent",
                      us[i], (unsigned long long)periods);
            if (dump) {
                static const char* ext[4] = {"in1", "in2", "outL", "outR"};
                for (int k = 0; k < 4; k++) {
                    std::ofstream f(std::string(dump) + std::to_string(i) + "." + ext[k], std::ios::binary);
                    f.write(reinterpret_cast<const char*>(feeds[i].rec[k].data()), (std::streamsize)(feeds[i].rec[k].size() * sizeof(float)));
                }
            }
        }
    } else {
        std::cin.get();
    }

    for (auto* c : instances) {
        for (int i = 0; i < 2; i++)
            if (auto* d = c->cc[i].device)
                if (d->isOpen) d->stop();
        if (c->isRunning()) c->stop();
        Log::info(c->name, "Average convolution runtime: %f ms", c->avgRuntime());
        delete c;
    }
    for (auto& kv : midiDevices) delete kv.second;
    return 0;
}
