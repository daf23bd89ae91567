// parse_dump <grammar> <argument>: what one of Convolution's static argument parsers (conv.h) makes of one argument, on one line:
// "ok" or "refused", the reason, then every member of the struct the parser fills, by name, whether it accepted or not (a refused
// argument leaves the struct as it was).  No engine call, no GPU.  tests/test_host_parse_cpu.py compares these lines with
// tests/golden/host_parse.json.  A member added to one of the structs gets a line here.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../cuda_audio_amd/host/conv.h"

static std::string line;

static void put(const char* name, const std::string& text) { line += std::string(" ") + name + "=" + text; }
static void f32(const char* name, float v) {
    char b[64];
    std::snprintf(b, sizeof(b), "%.9g", (double)v);
    put(name, b);
}
static void f64(const char* name, double v) {
    char b[64];
    std::snprintf(b, sizeof(b), "%.17g", v);
    put(name, b);
}
static void u64(const char* name, uint64_t v) {
    char b[64];
    std::snprintf(b, sizeof(b), "%" PRIu64, v);
    put(name, b);
}
static void flag(const char* name, bool v) { put(name, v ? "1" : "0"); }
static void str(const char* name, const std::string& v) {
    std::string q = "\"";
    for (char c : v) {
        if (c == '"' || c == '\\') q += '\\';
        q += c;
    }
    put(name, q + "\"");
}
template <typename T, size_t N>
static void f32s(const char* name, const T (&v)[N]) {
    for (size_t k = 0; k < N; k++) f32((std::string(name) + "[" + std::to_string(k) + "]").c_str(), v[k]);
}
template <size_t N>
static void f64s(const char* name, const double (&v)[N]) {
    for (size_t k = 0; k < N; k++) f64((std::string(name) + "[" + std::to_string(k) + "]").c_str(), v[k]);
}
template <size_t N>
static void flags(const char* name, const bool (&v)[N]) {
    for (size_t k = 0; k < N; k++) flag((std::string(name) + "[" + std::to_string(k) + "]").c_str(), v[k]);
}
static void f32v(const char* name, const std::vector<float>& v) {
    u64((std::string(name) + ".size").c_str(), v.size());
    for (size_t k = 0; k < v.size(); k++) f32((std::string(name) + "[" + std::to_string(k) + "]").c_str(), v[k]);
}

static void dump(const Convolution::IrTail& t) {
    u64("mode", (uint64_t)t.mode);
    f64("fadeSeconds", t.fadeSeconds);
    f64("lengthSeconds", t.lengthSeconds);
    u64("seed", t.seed);
    f32("width", t.width);
    flag("kneeAtMix", t.kneeAtMix);
    flag("widthFromIacc", t.widthFromIacc);
}
static void dump(const Convolution::IrPhase& p) {
    flag("minimum", p.minimum);
    f32("floorDb", p.floorDb);
    u64("overLog2", p.overLog2);
}
static void dump(const Convolution::IrFilter& f) {
    flag("on", f.on);
    flag("deconvolve", f.deconvolve);
    u64("channels", f.channels);
    f32("regDb", f.regDb);
    f64("keepSeconds", f.keepSeconds);
    str("path", f.path);
    u64("rate", f.rate);
    f32v("lr", f.lr);
}
static void dump(const Convolution::IrMatch& m) {
    flag("on", m.on);
    flag("flat", m.flat);
    flag("linear", m.linear);
    flag("link", m.link);
    f32("amount", m.amount);
    f32("boostDb", m.boostDb);
    f32("cutDb", m.cutDb);
    f64("octaves", m.octaves);
    f64("loHz", m.loHz);
    f64("hiHz", m.hiHz);
    f64("delaySeconds", m.delaySeconds);
    f32("tiltDb", m.tiltDb);
    str("path", m.path);
    u64("rate", m.rate);
    f32v("lr", m.lr);
}
static void dump(const Convolution::IrParts& p) {
    flag("on", p.on);
    flags("mute", p.mute);
    flags("swap", p.swap);
    flags("invert", p.invert);
    f32s("gainDb", p.gainDb);
    f32s("width", p.width);
    f32s("balance", p.balance);
    f64s("delaySeconds", p.delaySeconds);
    f64s("xfadeSeconds", p.xfadeSeconds);
    f64("onsetSeconds", p.onsetSeconds);
    f64("firstSeconds", p.firstSeconds);
    f64("splitSeconds", p.splitSeconds);
    flag("splitAtMix", p.splitAtMix);
}
static void dump(const Convolution::IrSynth& y, const std::string& in = "") {
    f64((in + "lengthSeconds").c_str(), y.lengthSeconds);
    f64((in + "t60Seconds").c_str(), y.t60Seconds);
    u64((in + "seed").c_str(), y.seed);
    f64((in + "startSeconds").c_str(), y.startSeconds);
    f64((in + "buildUpSeconds").c_str(), y.buildUpSeconds);
    f32((in + "late").c_str(), y.late);
    f32((in + "direct").c_str(), y.direct);
    u64((in + "early").c_str(), y.early);
    f64((in + "earlyFirstSeconds").c_str(), y.earlyFirstSeconds);
    f64((in + "earlyLastSeconds").c_str(), y.earlyLastSeconds);
    f32((in + "earlyGain").c_str(), y.earlyGain);
    f32((in + "width").c_str(), y.width);
}
static void dump(const Convolution::IrRoom& r) {
    f32s("size", r.size);
    f32s("source", r.source);
    f32s("receiver", r.receiver);
    f32s("beta", r.beta);
    f32("spacing", r.spacing);
    u64("axis", r.axis);
    f32("speed", r.speed);
    f32("gain", r.gain);
    u64("order", r.order);
    f64("lastSeconds", r.lastSeconds);
    flag("directional", r.directional);
    f32s("micPattern", r.micPattern);
    f32s("micAim", r.micAim);
    f32s("micTilt", r.micTilt);
    f32("sourcePattern", r.sourcePattern);
    f32("sourceAim", r.sourceAim);
    f32("sourceTilt", r.sourceTilt);
    flag("banded", r.banded);
    u64("nXovers", r.nXovers);
    u64("nBetas", r.nBetas);
    u64("nAir", r.nAir);
    f32s("xovers", r.xovers);
    f32s("betas", r.betas);
    f32s("air", r.air);
    flag("headed", r.headed);
    f32("headFacing", r.headFacing);
    f32("headRadius", r.headRadius);
    f32("headEars", r.headEars);
    f32("headShadow", r.headShadow);
    dump(r.late, "late.");
}
static void dump(const Convolution::IrPlate& p) {
    f64("lengthSeconds", p.lengthSeconds);
    f32s("size", p.size);
    f32("thickness", p.thickness);
    f32s("material", p.material);
    f32s("driver", p.driver);
    f32s("pickup[0]", p.pickup[0]);
    f32s("pickup[1]", p.pickup[1]);
    f32("low", p.low);
    f32("high", p.high);
    f32s("t60", p.t60);
    f32("damp", p.damp);
    f32("gain", p.gain);
    f64("lastSeconds", p.lastSeconds);
}
static void dump(const Convolution::IrSpring& s) {
    f64("lengthSeconds", s.lengthSeconds);
    u64("sections", s.sections);
    f32("transition", s.transition);
    f32("dispersion", s.dispersion);
    f32s("delayMs", s.delayMs);
    f32("t60", s.t60);
    f32("damping", s.damping);
    u64("lowpass", s.lowpass);
    f32("high", s.high);
    u64("highSections", s.highSections);
    f32("highDispersion", s.highDispersion);
    f32("highDelay", s.highDelay);
    f32("highT60", s.highT60);
    f32("stereo", s.stereo);
    f32("gain", s.gain);
    u64("points", s.points);
    f64("lastSeconds", s.lastSeconds);
}
static void dump(const Convolution::IrSweep& w) {
    str("recording", w.recording);
    f64("lengthSeconds", w.lengthSeconds);
    f32("f1", w.f1);
    f32("f2", w.f2);
    f32("amp", w.amp);
    f64("fadeInSeconds", w.fadeInSeconds);
    f64("fadeOutSeconds", w.fadeOutSeconds);
    f64("offsetSeconds", w.offsetSeconds);
    f64("irLengthSeconds", w.irLengthSeconds);
}
static void dump(const Convolution::DensityQuery& q) {
    f64("windowSeconds", q.windowSeconds);
    f64("hopSeconds", q.hopSeconds);
    f64("t60Seconds", q.t60Seconds);
    flag("autoT60", q.autoT60);
}
static void dump(const Convolution::IaccQuery& q) {
    f32v("bands", q.bands);
    f64("lagSeconds", q.lagSeconds);
    flag("lagGiven", q.lagGiven);
}
static void dump(const Convolution::StiQuery& q) { f32v("snrDb", q.snrDb); }
static void dump(const Convolution::ResponseQuery& q) { f64("smoothOctaves", q.smoothOctaves); }

template <typename T, typename Parse>
static int run(Parse parse) {
    T out;
    std::string why;
    const bool ok = parse(out, why);
    line = ok ? "ok" : "refused";
    str("why", why);
    dump(out);
    std::puts(line.c_str());
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "parse_dump <grammar> <argument>\n");
        return 2;
    }
    using C = Convolution;
    const std::string g = argv[1], arg = argv[2];
    if (g == "tail") return run<C::IrTail>([&](C::IrTail& o, std::string& w) { return C::parseTail(arg, o, w); });
    if (g == "phase") return run<C::IrPhase>([&](C::IrPhase& o, std::string& w) { return C::parsePhase(arg, o, w); });
    if (g == "filter") return run<C::IrFilter>([&](C::IrFilter& o, std::string& w) { return C::parseFilter(arg, o, w); });
    if (g == "match") return run<C::IrMatch>([&](C::IrMatch& o, std::string& w) { return C::parseMatch(arg, o, w); });
    if (g == "parts") return run<C::IrParts>([&](C::IrParts& o, std::string& w) { return C::parseParts(arg, o, w); });
    if (g == "synth") return run<C::IrSynth>([&](C::IrSynth& o, std::string& w) { return C::parseSynth(arg, o, w); });
    if (g == "room") return run<C::IrRoom>([&](C::IrRoom& o, std::string& w) { return C::parseRoom(arg, o, w); });
    if (g == "plate") return run<C::IrPlate>([&](C::IrPlate& o, std::string& w) { return C::parsePlate(arg, o, w); });
    if (g == "spring") return run<C::IrSpring>([&](C::IrSpring& o, std::string& w) { return C::parseSpring(arg, o, w); });
    if (g == "sweep") return run<C::IrSweep>([&](C::IrSweep& o, std::string& w) { return C::parseSweep(arg, o, w); });
    if (g == "density-window" || g == "density-hop" || g == "density-t60")
        return run<C::DensityQuery>([&](C::DensityQuery& o, std::string& w) { return C::parseDensity("--ir-" + g, arg, o, w); });
    if (g == "iacc-lag" || g == "iacc-bands") return run<C::IaccQuery>([&](C::IaccQuery& o, std::string& w) { return C::parseIacc("--ir-" + g, arg, o, w); });
    if (g == "sti-snr") return run<C::StiQuery>([&](C::StiQuery& o, std::string& w) { return C::parseSti(arg, o, w); });
    if (g == "response-smooth") return run<C::ResponseQuery>([&](C::ResponseQuery& o, std::string& w) { return C::parseResponse(arg, o, w); });
    std::fprintf(stderr, "parse_dump: no grammar '%s'\n", argv[1]);
    return 2;
}
