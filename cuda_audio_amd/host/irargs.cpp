// irargs.cpp — the text side of the IR options and index lines: Convolution's static parse* functions (conv.h).  One key=value
// grammar in two dialects, and per argument a table of rows (key, destination, bounds) plus what is truly its own: the leading
// positional fields, the named words, the keys whose value is a list, and the rules between keys.  No engine call and no member
// state: tests/stub/parse_dump.cpp links this file alone, and tests/test_host_parse_cpu.py pins what every argument parses to.
//
// The index-line dialect (synth:, room:, plate:, spring:, sweep:): fields separated by ':', the last an optional list of
// key=value items; a refusal names the text and the key, `'<text>' is no value for <key>`, or gives the form for an unknown key.
// The option dialect (--ir-tail, --ir-phase, --ir-filter, --ir-match, --ir-parts): every refusal is `<reason> (<form>)`, an item
// with an empty key or value is not key=value, and a value out of range is told its bounds.
#include <cmath>
#include <cstdlib>
#include <limits>

#include "conv.h"

namespace {

const double INF = std::numeric_limits<double>::infinity();

// The pieces of text between every sep, empty ones included (one piece for a text without sep)
std::vector<std::string> split(const std::string& text, char sep) {
    std::vector<std::string> pieces;
    for (size_t at = 0;;) {
        const size_t end = text.find(sep, at);
        pieces.push_back(text.substr(at, end == std::string::npos ? end : end - at));
        if (end == std::string::npos) return pieces;
        at = end + 1;
    }
}

// A finite number that fills the whole text
bool number(const std::string& text, double& v) {
    char* end = nullptr;
    v = std::strtod(text.c_str(), &end);
    return !text.empty() && end == text.c_str() + text.size() && std::isfinite(v);
}

// The same read as a float (a text that overflows a float is refused)
bool number(const std::string& text, float& v) {
    char* end = nullptr;
    v = std::strtof(text.c_str(), &end);
    return !text.empty() && end == text.c_str() + text.size() && std::isfinite(v);
}

// A whole number >= 0 in `base` (0: by its prefix) that fills the whole text
bool number(const std::string& text, int base, uint64_t& v) {
    char* end = nullptr;
    v = std::strtoull(text.c_str(), &end, base);
    return !text.empty() && text[0] != '-' && end == text.c_str() + text.size();
}

// `count` numbers >= lo separated by sep that fill the whole text
bool numbers(const std::string& text, char sep, size_t count, double lo, float* v) {
    const std::vector<std::string> pieces = split(text, sep);
    if (pieces.size() != count) return false;
    for (size_t k = 0; k < count; k++) {
        double x;
        if (!number(pieces[k], x) || x < lo) return false;
        v[k] = (float)x;
    }
    return true;
}

// One to `most` numbers separated by '/', each as a float within [lo, hi]
bool upTo(const std::string& text, size_t most, double lo, double hi, float* v, uint32_t& count) {
    count = (uint32_t)split(text, '/').size();
    if (count > most || !numbers(text, '/', count, -INF, v)) return false;
    for (uint32_t k = 0; k < count; k++)
        if (!((double)v[k] >= lo && (double)v[k] <= hi)) return false;
    return true;
}

// A comma-separated list of at most `most` floats, each within [lo, hi] (above lo when `open`)
bool floats(const std::string& arg, size_t most, float lo, bool open, float hi, std::vector<float>& out) {
    for (const std::string& piece : split(arg, ',')) {
        float x;
        if (!number(piece, x) || x < lo || (open && x == lo) || x > hi || out.size() >= most) return false;
        out.push_back(x);
    }
    return true;
}

// A key of a grammar: where its number goes and the bounds it has to keep
struct Row {
    const char* key;
    enum Kind { F32, F64, Whole } kind;
    void* to;
    double lo, hi;
    bool open;            // lo itself is out of bounds
    const char* outside;  // option dialect: what follows "<key> <value>" in the refusal of a value out of bounds
    bool* used;           // set when the key is given (IrRoom's directional, banded, headed)
};
Row f32(const char* key, float& to, double lo, double hi, const char* outside = nullptr, bool* used = nullptr) {
    return {key, Row::F32, &to, lo, hi, false, outside, used};
}
Row f64(const char* key, double& to, double lo, double hi, const char* outside = nullptr) { return {key, Row::F64, &to, lo, hi, false, outside, nullptr}; }
Row whole(const char* key, unsigned& to, double hi) { return {key, Row::Whole, &to, 0.0, hi, false, nullptr, nullptr}; }
Row above(Row row) {  // (lo, hi] in place of [lo, hi]
    row.open = true;
    return row;
}

template <size_t N>
const Row* find(const Row (&rows)[N], const std::string& key) {
    for (const Row& r : rows)
        if (key == r.key) return &r;
    return nullptr;
}

// v into the row's destination; false when it is out of the row's bounds
bool put(const Row& r, double v) {
    if (v < r.lo || v > r.hi || (r.open && v == r.lo) || (r.kind == Row::Whole && v != std::floor(v))) return false;
    if (r.kind == Row::F32) *static_cast<float*>(r.to) = (float)v;
    else if (r.kind == Row::F64) *static_cast<double*>(r.to) = v;
    else *static_cast<unsigned*>(r.to) = (unsigned)v;
    if (r.used) *r.used = true;
    return true;
}

// What a key's own code says of an item: not one of its keys, a value it refuses, or taken
enum Odd { NotMine, Bad, Taken };

// ---- the index-line dialect

// The fields of an index line: `word`, then `least` - 1 positional fields, then at most one list.  `what` begins the refusal.
bool fields(const std::string& line, const char* word, size_t least, const char* what, const char* form, std::vector<std::string>& parts, std::string& why) {
    parts = split(line, ':');
    if (parts.size() >= least && parts.size() <= least + 1 && parts[0] == word) return true;
    why = std::string(what) + form;
    return false;
}

bool lengthSeconds(const std::string& text, double& v, std::string& why) {
    if (number(text, v) && v > 0.0) return true;
    why = "LENGTH_S '" + text + "' is not a length in seconds, > 0";
    return false;
}

// The items of an index line's list, the field after the `least` leading ones.  Every comma separates two items; with
// `commaValues` (plate:, spring:) only a comma that key= follows does, or one at either end of the list or next to another, and
// any other belongs to the value before it (size=LX,LY).
bool listItems(const std::vector<std::string>& parts, size_t least, bool commaValues, const char* form, std::vector<std::string>& items, std::string& why) {
    if (parts.size() == least) return true;
    if (parts[least].empty()) {
        why = std::string("nothing after the last colon: ") + form;
        return false;
    }
    for (const std::string& piece : split(parts[least], ',')) {
        if (!commaValues || piece.find('=') != std::string::npos || items.empty() || piece.empty()) items.push_back(piece);
        else items.back() += "," + piece;
    }
    return true;
}

// Every item through `odd` (the grammar's own keys) and then the rows
template <size_t N, typename OddKeys>
bool indexItems(const std::vector<std::string>& items, const Row (&rows)[N], const char* form, std::string& why, OddKeys odd) {
    for (const std::string& item : items) {
        const size_t eq = item.find('=');
        if (eq == std::string::npos) {
            why = "'" + item + "' is not key=value";
            return false;
        }
        const std::string key = item.substr(0, eq), text = item.substr(eq + 1);
        Odd took = odd(key, text, item);
        if (took == NotMine) {
            const Row* row = find(rows, key);
            if (!row) {
                why = "unknown key '" + key + "': " + form;
                return false;
            }
            double v;
            took = number(text, v) && put(*row, v) ? Taken : Bad;
        }
        if (took == Bad) {
            why = "'" + text + "' is no value for " + key;
            return false;
        }
    }
    return true;
}

Odd noOddKeys(const std::string&, const std::string&, const std::string&) { return NotMine; }

// ---- the option dialect

struct Refusal {
    const char* form;
    std::string& why;
    bool operator()(const std::string& reason) const {
        why = reason + " (" + form + ")";
        return false;
    }
};

// An item of an option's list as key and value, neither empty
bool keyValue(const std::string& item, std::string& key, std::string& val) {
    const size_t eq = item.find('=');
    if (item.empty() || eq == std::string::npos || eq == 0 || eq + 1 == item.size()) return false;
    key = item.substr(0, eq), val = item.substr(eq + 1);
    return true;
}

// What follows the first field of an option, when anything does: every item through `odd` (which gives the reason for a value it
// refuses) and then the rows.  `numberFirst`: a value that is no number is told so before its key is looked up (--ir-phase,
// --ir-tail); without, an unknown key is named first (--ir-filter, --ir-match).
template <size_t N, typename OddKeys>
bool optionItems(const std::string& arg, const Row (&rows)[N], bool numberFirst, const Refusal& fail, OddKeys odd) {
    const size_t colon = arg.find(':');
    if (colon == std::string::npos) return true;
    if (colon + 1 == arg.size()) return fail("an empty list");
    for (const std::string& item : split(arg.substr(colon + 1), ',')) {
        std::string key, val, reason;
        if (!keyValue(item, key, val)) return fail("'" + item + "' is not key=value");
        const Odd took = odd(key, val, reason);
        if (took == Bad) return fail(reason);
        if (took == Taken) continue;
        const Row* row = find(rows, key);
        double v;
        if (!row && !numberFirst) return fail("no such key '" + key + "'");
        if (!number(val, v)) return fail("'" + val + "' of " + key + " is not a number");
        if (!row) return fail("no such key '" + key + "'");
        if (!put(*row, v)) return fail(key + " " + val + row->outside);
    }
    return true;
}

// key=val where the value is one of `words`: its index into `to`, or the reason
template <size_t N, typename T>
Odd word(const std::string& val, const char* const (&words)[N], const char* reason, T& to, std::string& why) {
    for (size_t k = 0; k < N; k++)
        if (val == words[k]) {
            to = (T)k;
            return Taken;
        }
    why = std::string(reason) + ", not '" + val + "'";
    return Bad;
}

}  // namespace

bool Convolution::parseTail(const std::string& arg, IrTail& out, std::string& why) {
    const Refusal fail{"cut|extend[:key=value,...] with keys fade, length, seed, width, knee", why};
    static const char* const knees[] = {"floor", "mix"};
    const std::string mode = arg.substr(0, arg.find(':'));
    IrTail t;
    if (mode == "cut") t.mode = IrTail::Cut;
    else if (mode == "extend") t.mode = IrTail::Extend;
    else return fail("the mode is cut or extend, not '" + mode + "'");
    const Row width = f32("width", t.width, 0.0, 1.0, " outside [0, 1]");
    const Row rows[] = {f64("fade", t.fadeSeconds, 0.0, 4000.0, " s outside [0, 4000]"), f64("length", t.lengthSeconds, 0.0, 4000.0, " s outside [0, 4000]"), width};
    const auto odd = [&](const std::string& key, const std::string& val, std::string& reason) {
        if (key == "knee") return word(val, knees, "knee is floor or mix", t.kneeAtMix, reason);
        if (key == "seed") {
            reason = "seed '" + val + "' is not a number >= 0";
            return number(val, 10, t.seed) ? Taken : Bad;
        }
        if (key == width.key) return (t.widthFromIacc = val == "iacc") ? Taken : NotMine;  // (iacc, or the row's number, which takes an earlier iacc back)
        return NotMine;
    };
    if (!optionItems(arg, rows, true, fail, odd)) return false;
    if (t.kneeAtMix && t.mode != IrTail::Extend) return fail("knee=mix slides the levels of an extended tail: the mode must be extend");
    if (t.widthFromIacc && t.mode != IrTail::Extend) return fail("width=iacc is the width of an extended tail's noise: the mode must be extend");
    out = t;
    return true;
}

bool Convolution::parsePhase(const std::string& arg, IrPhase& out, std::string& why) {
    const Refusal fail{"minimum[:key=value,...] with keys floor, over", why};
    const std::string mode = arg.substr(0, arg.find(':'));
    IrPhase p;
    if (mode != "minimum") return fail("the mode is minimum, not '" + mode + "'");
    p.minimum = true;
    const Row rows[] = {f32("floor", p.floorDb, 40.0, 300.0, " dB outside [40, 300]")};
    const auto odd = [&](const std::string& key, const std::string& val, std::string& reason) {
        double v;
        if (key != "over" || !number(val, v)) return NotMine;  // (what is no number is told so whatever its key)
        reason = "over " + val + " is not a power of two from 2 to 64";
        for (p.overLog2 = 1; p.overLog2 <= 6; p.overLog2++)
            if ((double)(1u << p.overLog2) == v) return Taken;
        return Bad;
    };
    if (!optionItems(arg, rows, true, fail, odd)) return false;
    out = p;
    return true;
}

bool Convolution::parseFilter(const std::string& arg, IrFilter& out, std::string& why) {
    const Refusal fail{"FILE.wav[:key=value,...] with keys op, channels, reg, keep", why};
    static const char* const ops[] = {"convolve", "deconvolve"};
    static const char* const channels[] = {"stereo", "left", "mid"};
    IrFilter f;
    f.path = arg.substr(0, arg.find(':'));
    if (f.path.empty()) return fail("no file");
    f.on = true;
    const Row rows[] = {f32("reg", f.regDb, 20.0, 200.0, " dB outside [20, 200]"), above(f64("keep", f.keepSeconds, 0.0, 3600.0, " s outside (0, 3600]"))};
    const auto odd = [&](const std::string& key, const std::string& val, std::string& reason) {
        if (key == "op") return word(val, ops, "op is convolve or deconvolve", f.deconvolve, reason);
        if (key == "channels") return word(val, channels, "channels is stereo, left or mid", f.channels, reason);
        return NotMine;
    };
    if (!optionItems(arg, rows, false, fail, odd)) return false;
    out = f;
    return true;
}

bool Convolution::parseMatch(const std::string& arg, IrMatch& out, std::string& why) {
    const Refusal fail{"FILE.wav|flat[:key=value,...] with keys amount, boost, cut, smooth, lo, hi, link, phase, delay, tilt", why};
    static const char* const phases[] = {"minimum", "linear"};
    static const char* const links[] = {"0", "1"};
    IrMatch m;
    m.path = arg.substr(0, arg.find(':'));
    if (m.path.empty()) return fail("no file");
    m.flat = m.path == "flat";
    m.on = true;
    const Row rows[] = {f32("amount", m.amount, 0.0, 1.0, " outside [0, 1]"),
                        f32("boost", m.boostDb, 0.0, 60.0, " dB outside [0, 60]"),
                        f32("cut", m.cutDb, 0.0, 60.0, " dB outside [0, 60]"),
                        f64("smooth", m.octaves, 1.0 / 24.0, 2.0, " octaves outside [1/24, 2]"),
                        f64("lo", m.loHz, 1.0, 192000.0, " Hz outside [1, 192000]"),
                        f64("hi", m.hiHz, 1.0, 192000.0, " Hz outside [1, 192000]"),
                        f64("delay", m.delaySeconds, 0.0, 10.0, " s outside [0, 10]"),
                        f32("tilt", m.tiltDb, -12.0, 12.0, " dB per octave outside [-12, 12]")};
    const auto odd = [&](const std::string& key, const std::string& val, std::string& reason) {
        if (key == "phase") return word(val, phases, "phase is minimum or linear", m.linear, reason);
        if (key == "link") return word(val, links, "link is 0 or 1", m.link, reason);
        return NotMine;
    };
    if (!optionItems(arg, rows, false, fail, odd)) return false;
    if (m.hiHz != 0.0 && !(m.hiHz > m.loHz)) return fail("hi is not above lo");
    out = m;
    return true;
}

bool Convolution::parseParts(const std::string& arg, IrParts& out, std::string& why) {
    const Refusal fail{"key=value,... with keys direct, early, late, split, first, onset, xfade, delay, width, balance, swap, invert", why};
    static const char* const names[3] = {"direct", "early", "late"};
    if (arg.empty()) return fail("an empty list");
    IrParts p;
    p.on = true;
    // `count` numbers joined by ':' (or one for all when `one`), each within [lo, hi]
    const auto numbers = [](const std::string& val, size_t count, bool one, double lo, double hi, double* v) {
        const std::vector<std::string> texts = split(val, ':');
        if (texts.size() != count && !(one && texts.size() == 1)) return false;
        for (size_t k = 0; k < count; k++)
            if (!number(texts[texts.size() == 1 ? 0 : k], v[k]) || v[k] < lo || v[k] > hi) return false;
        return true;
    };
    const auto part = [](const std::string& name) {
        int k = 0;
        while (k < 3 && name != names[k]) k++;
        return k;
    };
    for (const std::string& item : split(arg, ',')) {
        const std::string name = item.substr(0, item.find('='));
        bool* const flags = name == "swap" ? p.swap : name == "invert" ? p.invert : nullptr;
        if (flags && item == name) {  // (alone: all three parts)
            for (int k = 0; k < 3; k++) flags[k] = true;
            continue;
        }
        std::string key, val;
        if (!keyValue(item, key, val)) return fail("'" + item + "' is not key=value");
        double v[3];
        if (const int k = part(key); k < 3) {
            p.mute[k] = val == "off";
            if (p.mute[k]) continue;
            if (!numbers(val, 1, true, -120.0, 24.0, v)) return fail(key + " is a gain in dB within [-120, 24] or off, not '" + val + "'");
            p.gainDb[k] = (float)v[0];
        } else if (key == "split") {
            p.splitAtMix = val == "mix";
            if (!p.splitAtMix && !numbers(val, 1, true, 0.0, 100.0, &p.splitSeconds)) return fail("split is a time in seconds within [0, 100] or mix, not '" + val + "'");
        } else if (double* const seconds = key == "first" ? &p.firstSeconds : key == "onset" ? &p.onsetSeconds : nullptr) {
            if (!numbers(val, 1, true, 0.0, 100.0, seconds)) return fail(key + " is a time in seconds within [0, 100], not '" + val + "'");
        } else if (key == "xfade") {
            if (!numbers(val, 2, false, 0.0, 100.0, p.xfadeSeconds)) return fail("xfade is S:S, two times in seconds within [0, 100], not '" + val + "'");
        } else if (key == "delay") {
            if (!numbers(val, 3, false, -10.0, 10.0, p.delaySeconds)) return fail("delay is S:S:S, three times in seconds within [-10, 10], not '" + val + "'");
        } else if (key == "width") {
            if (!numbers(val, 3, true, 0.0, 2.0, v)) return fail("width is one number or W:W:W within [0, 2], not '" + val + "'");
            for (int k = 0; k < 3; k++) p.width[k] = (float)v[k];
        } else if (key == "balance") {
            if (!numbers(val, 3, true, -1.0, 1.0, v)) return fail("balance is one number or B:B:B within [-1, 1], not '" + val + "'");
            for (int k = 0; k < 3; k++) p.balance[k] = (float)v[k];
        } else if (flags) {
            for (const std::string& one : split(val, ':')) {
                if (part(one) == 3) return fail(key + " names parts (direct, early, late) joined by ':', not '" + val + "'");
                flags[part(one)] = true;
            }
        } else
            return fail("no such key '" + key + "'");
    }
    if (!p.splitAtMix && p.splitSeconds < p.firstSeconds) return fail("split is before first");
    if (p.mute[0] && p.mute[1] && p.mute[2]) return fail("every part is off");
    out = p;
    return true;
}

bool Convolution::parseSynth(const std::string& line, IrSynth& out, std::string& why) {
    static const char* form = "synth:LENGTH_S:T60_S[:key=value,...] with keys seed, start, buildup, late, direct, early, efirst, elast, egain, width";
    std::vector<std::string> parts, items;
    IrSynth y;
    if (!fields(line, "synth", 3, "a generated IR is ", form, parts, why) || !lengthSeconds(parts[1], y.lengthSeconds, why)) return false;
    if (!number(parts[2], y.t60Seconds) || y.t60Seconds < 0.0) {
        why = "T60_S '" + parts[2] + "' is not a decay time in seconds, >= 0 (0 = no decay)";
        return false;
    }
    const Row rows[] = {whole("early", y.early, MC_SYNTH_MAX_EARLY), f32("late", y.late, 0.0, INF), f32("direct", y.direct, -INF, INF),
                        f32("egain", y.earlyGain, -INF, INF), f32("width", y.width, 0.0, 1.0), f64("start", y.startSeconds, 0.0, INF),
                        f64("buildup", y.buildUpSeconds, 0.0, INF), f64("efirst", y.earlyFirstSeconds, 0.0, INF), f64("elast", y.earlyLastSeconds, 0.0, INF)};
    const auto odd = [&](const std::string& key, const std::string& text, const std::string&) {
        return key != "seed" ? NotMine : number(text, 0, y.seed) ? Taken : Bad;
    };
    if (!listItems(parts, 3, false, form, items, why) || !indexItems(items, rows, form, why, odd)) return false;
    if (y.early && y.earlyLastSeconds < y.earlyFirstSeconds) {
        why = "elast is before efirst";
        return false;
    }
    out = y;
    return true;
}

// A microphone pattern by name or as alpha in [0, 1]
static bool pattern(const std::string& text, float& v) {
    static const struct {
        const char* name;
        float alpha;
    } named[] = {{"omni", 1.0f}, {"subcardioid", 0.75f}, {"cardioid", 0.5f}, {"supercardioid", 0.366f}, {"hypercardioid", 0.25f}, {"fig8", 0.0f}};
    for (const auto& p : named)
        if (text == p.name) {
            v = p.alpha;
            return true;
        }
    double x;
    if (!number(text, x) || x < 0.0 || x > 1.0) return false;
    v = (float)x;
    return true;
}

// One value for both receivers, or left/right: each an angle within [-limit, limit], or a pattern with limit 0
static bool leftRight(const std::string& text, double limit, float* v) {
    const size_t slash = text.find('/');
    const std::string one[2] = {text.substr(0, slash), slash == std::string::npos ? text : text.substr(slash + 1)};
    for (int c = 0; c < 2; c++) {
        double x;
        if (limit == 0.0 ? !pattern(one[c], v[c]) : !number(one[c], x) || std::fabs(x) > limit) return false;
        if (limit != 0.0) v[c] = (float)x;
    }
    return true;
}

bool Convolution::parseRoom(const std::string& line, IrRoom& out, std::string& why) {
    static const char* form =
        "room:LENGTH_S:LX,LY,LZ:SX,SY,SZ:RX,RY,RZ[:key=value,...] with keys beta (one value, or six separated by '/'), order, spacing, axis (x|y|z), "
        "speed, gain, last, mic (omni|subcardioid|cardioid|supercardioid|hypercardioid|fig8 or a number in [0, 1]; P or P/P), aim and tilt (degrees; "
        "one value or L/R), src, srcaim, srctilt, xover (HZ[/HZ[/HZ]]), betas (one value per band, separated by '/'), air (dB per metre: one value, or one "
        "per band), head (the azimuth the listener faces, degrees), headradius (metres), ears (degrees from the facing direction), shadow ([0, 1]), "
        "t60 and synth:'s keys";
    static const char* const axes[] = {"x", "y", "z"};
    std::vector<std::string> parts, items;
    IrRoom room;
    double length = 0.0;
    if (!fields(line, "room", 5, "a room is ", form, parts, why) || !lengthSeconds(parts[1], length, why)) return false;
    const char* triple[3] = {"LX,LY,LZ", "SX,SY,SZ", "RX,RY,RZ"};
    float* slot[3] = {room.size, room.source, room.receiver};
    for (int k = 0; k < 3; k++)
        if (!numbers(parts[2 + k], ',', 3, -INF, slot[k])) {
            why = std::string(triple[k]) + " '" + parts[2 + k] + "' is not three numbers in metres";
            return false;
        }
    const Row rows[] = {whole("order", room.order, MC_ROOM_MAX_ORDER), f32("spacing", room.spacing, 0.0, INF), f32("speed", room.speed, 0.0, INF),
                        f32("gain", room.gain, 0.0, INF), f64("last", room.lastSeconds, 0.0, INF),
                        f32("srcaim", room.sourceAim, -360.0, 360.0, nullptr, &room.directional),
                        f32("srctilt", room.sourceTilt, -90.0, 90.0, nullptr, &room.directional),
                        f32("head", room.headFacing, -360.0, 360.0, nullptr, &room.headed),
                        f32("headradius", room.headRadius, 0.05, 0.15, nullptr, &room.headed),
                        f32("ears", room.headEars, 60.0, 120.0, nullptr, &room.headed),
                        f32("shadow", room.headShadow, 0.0, 1.0, nullptr, &room.headed)};
    std::string betasText, airText, unused, t60 = "0", synthKeys = "late=0,direct=0";  // (the room supplies the direct sound; a later late= or direct= wins)
    // (a value that is refused ends the parse, so directional and banded are only ever left set)
    const auto odd = [&](const std::string& key, const std::string& text, const std::string& item) {
        bool good;
        double v;
        if (key == "beta") {
            good = numbers(text, '/', 6, -INF, room.beta);
            if (!good && (good = number(text, v)))
                for (float& b : room.beta) b = (float)v;
        } else if (key == "axis") {
            return word(text, axes, "", room.axis, unused);
        } else if (key == "t60") {
            good = number(text, v) && v >= 0.0;
            t60 = text;
        } else if (key == "mic") {
            good = room.directional = leftRight(text, 0.0, room.micPattern);
        } else if (key == "aim") {
            good = room.directional = leftRight(text, 360.0, room.micAim);
        } else if (key == "tilt") {
            good = room.directional = leftRight(text, 90.0, room.micTilt);
        } else if (key == "src") {
            good = room.directional = pattern(text, room.sourcePattern);
        } else if (key == "xover") {
            good = room.banded = upTo(text, MC_DAMP_MAX_XOVERS, 10.0, 172800.0, room.xovers, room.nXovers);  // (the engine checks them against the client's rate)
            for (uint32_t k = 1; good && k < room.nXovers; k++) good = room.xovers[k] > room.xovers[k - 1];
        } else if (key == "betas") {
            good = room.banded = upTo(betasText = text, MC_DAMP_MAX_XOVERS + 1, -1.0, 1.0, room.betas, room.nBetas);
        } else if (key == "air") {
            good = room.banded = upTo(airText = text, MC_DAMP_MAX_XOVERS + 1, 0.0, 1.0, room.air, room.nAir);
        } else {
            if (find(rows, key)) return NotMine;
            synthKeys += "," + item;  // (the late field's: parseSynth names an unknown key)
            return Taken;
        }
        return good ? Taken : Bad;
    };
    if (!listItems(parts, 5, false, form, items, why) || !indexItems(items, rows, form, why, odd)) return false;
    // (the keys come in any order: the counts are compared once every key has been read)
    if (room.nBetas && room.nBetas != room.nXovers + 1) {
        why = "'" + betasText + "' is no value for betas: one value for each of the " + std::to_string(room.nXovers + 1) + " bands xover cuts";
        return false;
    }
    if (room.nAir > 1 && room.nAir != room.nXovers + 1) {
        why = "'" + airText + "' is no value for air: one value, or one for each of the " + std::to_string(room.nXovers + 1) + " bands xover cuts";
        return false;
    }
    if (!parseSynth("synth:" + parts[1] + ":" + t60 + ":" + synthKeys, room.late, why)) {
        const size_t at = why.find("synth:LENGTH_S");
        if (at != std::string::npos) why = why.substr(0, at) + form;
        return false;
    }
    out = room;
    return true;
}

bool Convolution::parsePlate(const std::string& line, IrPlate& out, std::string& why) {
    static const char* form =
        "plate:LENGTH_S[:key=value,...] with keys size=LX,LY (metres), thick=MM, material=steel|E/RHO/NU (GPa, kg/m^3, Poisson's ratio), drive=X,Y, "
        "pick=X,Y/X,Y (left/right), low=HZ, high=HZ, t60=LO/HI (seconds towards 0 Hz and at damp; 0 = no loss), damp=HZ, gain, last=S";
    std::vector<std::string> parts, items;
    IrPlate plate;
    if (!fields(line, "plate", 2, "a plate is ", form, parts, why) || !lengthSeconds(parts[1], plate.lengthSeconds, why)) return false;
    const Row rows[] = {f32("thick", plate.thickness, 0.0, INF), f32("low", plate.low, 0.0, INF), f32("high", plate.high, 0.0, INF),
                        f32("damp", plate.damp, 0.0, INF), f32("gain", plate.gain, 0.0, INF), f64("last", plate.lastSeconds, 0.0, INF)};
    const auto odd = [&](const std::string& key, const std::string& text, const std::string&) {
        bool good;
        if (key == "size") {
            good = numbers(text, ',', 2, 0.0, plate.size);
        } else if (key == "drive") {
            good = numbers(text, ',', 2, 0.0, plate.driver);
        } else if (key == "pick") {
            const size_t slash = text.find('/');
            good = slash != std::string::npos && numbers(text.substr(0, slash), ',', 2, 0.0, plate.pickup[0]) &&
                   numbers(text.substr(slash + 1), ',', 2, 0.0, plate.pickup[1]);
        } else if (key == "material") {
            good = numbers(text == "steel" ? "200/7850/0.3" : text, '/', 3, 0.0, plate.material);  // (GPa, kg/m^3, Poisson's ratio)
        } else if (key == "t60") {
            good = numbers(text, '/', 2, 0.0, plate.t60);
        } else
            return NotMine;
        return good ? Taken : Bad;
    };
    if (!listItems(parts, 2, true, form, items, why) || !indexItems(items, rows, form, why, odd)) return false;
    out = plate;
    return true;
}

bool Convolution::parseSpring(const std::string& line, IrSpring& out, std::string& why) {
    static const char* form =
        "spring:LENGTH_S[:key=value,...] with keys sections, fc=HZ (the transition), a (the dispersion), delay=MS[,MS[,MS]] (one per spring), t60=S, damping, "
        "lowpass=ORDER, high (the high chirps' gain), highsections, higha, highdelay (a part of the period), hight60=S, stereo, gain, points (log2 of the "
        "transform's size), last=S";
    std::vector<std::string> parts, items;
    IrSpring spring;
    if (!fields(line, "spring", 2, "a spring is ", form, parts, why) || !lengthSeconds(parts[1], spring.lengthSeconds, why)) return false;
    const Row rows[] = {
        whole("sections", spring.sections, 1e6), whole("lowpass", spring.lowpass, 1e6), whole("highsections", spring.highSections, 1e6),
        whole("points", spring.points, 1e6), f32("fc", spring.transition, 0.0, INF), f32("a", spring.dispersion, 0.0, INF),
        f32("t60", spring.t60, 0.0, INF), f32("damping", spring.damping, 0.0, INF), f32("high", spring.high, 0.0, INF),
        f32("highdelay", spring.highDelay, 0.0, INF), f32("hight60", spring.highT60, 0.0, INF), f32("stereo", spring.stereo, 0.0, INF),
        f32("gain", spring.gain, 0.0, INF), f64("last", spring.lastSeconds, 0.0, INF),
        f32("higha", spring.highDispersion, -INF, 0.0)};  // (the one key whose value is at most 0)
    const auto odd = [&](const std::string& key, const std::string& text, const std::string&) {
        if (key != "delay") return NotMine;  // one to three periods in milliseconds, > 0; the springs not named are absent
        const std::vector<std::string> ms = split(text, ',');
        for (size_t k = 0; k < 3; k++) {
            double v = 0.0;
            if (k < ms.size() && (!number(ms[k], v) || !(v > 0.0))) return Bad;
            spring.delayMs[k] = (float)v;
        }
        return ms.size() <= 3 ? Taken : Bad;
    };
    if (!listItems(parts, 2, true, form, items, why) || !indexItems(items, rows, form, why, odd)) return false;
    out = spring;
    return true;
}

bool Convolution::parseSweep(const std::string& line, IrSweep& out, std::string& why) {
    static const char* form = "sweep:RECORDING.wav:LENGTH_S:F1:F2[:key=value,...] with keys amp, fadein, fadeout, offset, length";
    std::vector<std::string> parts, items;
    IrSweep w;
    if (!fields(line, "sweep", 5, "a captured IR is ", form, parts, why)) return false;
    w.recording = parts[1];
    if (w.recording.empty()) {
        why = std::string("no file name: ") + form;
        return false;
    }
    double f1 = 0.0, f2 = 0.0;
    if (!lengthSeconds(parts[2], w.lengthSeconds, why)) return false;
    if (!number(parts[3], f1) || !(f1 >= 1.0)) {
        why = "F1 '" + parts[3] + "' is not a frequency in Hz, >= 1";
        return false;
    }
    if (!number(parts[4], f2) || !(f2 > f1)) {
        why = "F2 '" + parts[4] + "' is not a frequency in Hz above F1";
        return false;
    }
    w.f1 = (float)f1;
    w.f2 = (float)f2;
    const Row rows[] = {above(f32("amp", w.amp, 0.0, INF)), f64("fadein", w.fadeInSeconds, 0.0, INF), f64("fadeout", w.fadeOutSeconds, 0.0, INF),
                        f64("length", w.irLengthSeconds, 0.0, INF), f64("offset", w.offsetSeconds, -INF, INF)};
    if (!listItems(parts, 5, false, form, items, why) || !indexItems(items, rows, form, why, noOddKeys)) return false;
    if (w.fadeInSeconds + w.fadeOutSeconds > w.lengthSeconds) {
        why = "fadein and fadeout are longer than the sweep";
        return false;
    }
    out = w;
    return true;
}

bool Convolution::parseDensity(const std::string& option, const std::string& arg, DensityQuery& out, std::string& why) {
    const bool t60 = option == "--ir-density-t60";
    if (t60 && arg == "auto") {
        out.autoT60 = true, out.t60Seconds = 0.0;
        return true;
    }
    double v;
    if (!number(arg, v) || !(v > 0.0) || v > 4000.0) {
        why = "takes a time in seconds, > 0 and at most 4000" + std::string(t60 ? ", or auto" : "");
        return false;
    }
    if (option == "--ir-density-window") out.windowSeconds = v;
    else if (option == "--ir-density-hop") out.hopSeconds = v;
    else out.t60Seconds = v, out.autoT60 = false;
    return true;
}

bool Convolution::parseIacc(const std::string& option, const std::string& arg, IaccQuery& out, std::string& why) {
    if (option == "--ir-iacc-lag") {
        double v;
        if (!number(arg, v) || v < 0.0 || v > 1.0) {
            why = "takes a time in seconds, >= 0 and at most 1";
            return false;
        }
        out.lagSeconds = v, out.lagGiven = true;
        return true;
    }
    std::vector<float> bands;
    if (!floats(arg, MC_DECAY_MAX_BANDS, 0.f, true, (float)INF, bands)) {
        why = "takes HZ[,HZ...], each > 0, at most 10";
        return false;
    }
    out.bands = bands;
    return true;
}

bool Convolution::parseSti(const std::string& arg, StiQuery& out, std::string& why) {
    std::vector<float> snr;
    if (!floats(arg, MC_STI_MAX_BANDS, -60.f, false, 120.f, snr)) {
        why = "takes DB[,DB...]: one signal-to-noise ratio for all seven octaves or one per octave from 125 Hz up, each in [-60, 120]";
        return false;
    }
    if (snr.size() != 1 && snr.size() != MC_STI_MAX_BANDS) {
        why = "takes one signal-to-noise ratio for all seven octaves or seven, one per octave";
        return false;
    }
    snr.resize(MC_STI_MAX_BANDS, snr[0]);
    out.snrDb = snr;
    return true;
}

const char* Convolution::stiRating(double sti) {
    if (std::isnan(sti)) return "none";
    return sti < 0.30 ? "bad" : sti < 0.45 ? "poor" : sti < 0.60 ? "fair" : sti < 0.75 ? "good" : "excellent";
}

bool Convolution::parseResponse(const std::string& arg, ResponseQuery& out, std::string& why) {
    double octaves;
    if (!number(arg, octaves) || octaves < 0.0 || octaves > 10.0) {
        why = "takes OCTAVES: the width the report's levels are smoothed over, in [0, 10]";
        return false;
    }
    out.smoothOctaves = octaves;
    return true;
}
