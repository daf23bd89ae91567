"""Float64 restatement of the noise-floor search of a loaded IR (mc_ir_floor, cuda_audio_amd/csrc/irfloor.hip.h): Lundeby's
method as include/mcconv.h states it.

Test infrastructure only: the product never imports it.  x = the n stored taps (float32 [n, 2]) as double, N = end ? min(end, n) : n;
  origin o, the channel sets and EDC[m], m in [o, N], EDC[N] = 0: ir_decay_np's steps 1, 3 and 4;
  row group 0: y = x.  With X >= 1 crossovers group j + 1 is band B_j of ir_damp_np's split of x[0 .. N) (sequential loops);
  per row, with n1 = N - o, cap = n1 // 16, tail = max(1, floor(tail_fraction n1)) and the float32 fields as double:
    means(w)   I = n1 // w, P_i = (EDC[o + i w] - EDC[o + (i + 1) w]) / w, D_i = 10 log10 P_i, t_i = o + i w + (w - 1) / 2;
    noise(a)   Nz = EDC[a] / (N - a), V = 10 log10 Nz; Nz = 0 ends the row with status 3, before anything is fitted;
    run(V)     ip = the first index of the largest P_i, iF = the first i >= ip with D_i < V + margin_db (I when none), R = [ip, iF);
    fit(S)     least squares of D_i over x_i = t_i - t_(min S): a, c = (sum y - a sum x) / |S|, crossing t_(min S) + (V - c) / a;
               status 2 when |S| < 2 or a is not a finite negative number;
    status 1   cap < 1 or E = EDC[o] = 0;
    first      w0 = min(window or floor(0.03 rate + 0.5), cap), V = noise(N - tail), fit(run(V)) over means(w0), tc = the crossing;
    interval   w = clamp(floor(-10 / (a per_decade) + 0.5), 1, cap), once; means(w);
    rounds     exactly `rounds` times: a_n = min(max(ceil(tc + margin_db / -a), o), N - tail), V = noise(a_n), R = run(V),
               S = {i in R : D_i <= V + margin_db + span_db} or R when that has fewer than 2 members, fit(S), tc_prev = tc, tc = the crossing;
    row        {E, Nz, tc, T = -60 / (a rate), 10 log10(max P_i / Nz), w, |tc - tc_prev|, status}.
`floor` also returns the margin of every discrete decision (see `margins`), which assert_margins bounds from below before
anything is compared with the device.
"""
import math

import numpy as np

import ir_damp_np
import ir_decay_np
from ir_decay_np import SETS

FIELDS = ("energy", "noise", "knee", "t", "peak_to_noise_db", "interval", "last_change", "status")
DEFAULTS = dict(window=0, tail_fraction=0.1, margin_db=10.0, span_db=20.0, per_decade=5, rounds=5)
NAN = float("nan")


def _f32(v):
    return float(np.float32(v))


def groups_of(x, xovers, rate):
    """[y of group 0, B_0 .. B_X] over the float64 taps x [N, 2]."""
    if not xovers:
        return [x]
    return [x] + ir_damp_np.bands(x, ir_damp_np.lowpasses(x, xovers, rate))


def edc_of(y, o):
    """EDC [3, N - o + 1] over taps o .. N of the row group's taps y [N, 2]; the last entry is EDC[N] = 0."""
    _, edc, _ = ir_decay_np.levels(y, o)
    return np.concatenate([edc, np.zeros((3, 1))], axis=1)


class _Row:
    def __init__(self, edc, o, N, rate, p):
        self.edc, self.o, self.N, self.rate, self.p = edc, o, N, rate, p
        self.n1 = N - o
        self.cap = self.n1 // 16
        self.tail = max(1, int(math.floor(p["tail_fraction"] * self.n1)))
        self.margins = dict(margin=[], span=[], peak=[], interval=[], ceil=[])

    def at(self, m):
        return float(self.edc[m - self.o])

    def means(self, w):
        I = self.n1 // w
        e = self.edc[np.arange(I + 1, dtype=np.int64) * w]
        self.P = (e[:-1] - e[1:]) / float(w)
        with np.errstate(divide="ignore"):
            self.D = 10.0 * np.log10(self.P)
        self.t = self.o + np.arange(I, dtype=np.float64) * w + (w - 1) / 2.0
        self.w = w
        top = np.sort(self.P)[::-1]
        if top.size > 1 and top[0] > 0.0 and top[1] > 0.0:
            self.margins["peak"].append(10.0 * math.log10(top[0] / top[1]))

    def noise(self, a):
        self.Nz = self.at(a) / float(self.N - a)
        self.V = 10.0 * math.log10(self.Nz) if self.Nz > 0.0 else -math.inf
        return self.Nz > 0.0

    def run(self, span):
        p = self.p
        ip = int(np.argmax(self.P))
        rest = self.D[ip:]
        fin = rest[np.isfinite(rest)]
        self.margins["margin"].append(float(np.abs(fin - (self.V + p["margin_db"])).min()) if fin.size else math.inf)
        below = np.nonzero(rest < self.V + p["margin_db"])[0]
        iF = ip + int(below[0]) if below.size else len(self.D)
        S = np.arange(ip, iF)
        if span:
            self.margins["span"].append(float(np.abs(fin - (self.V + p["margin_db"] + p["span_db"])).min()) if fin.size else math.inf)
            low = S[self.D[S] <= self.V + p["margin_db"] + p["span_db"]]
            if low.size >= 2:
                S = low
        return S

    def fit(self, S):
        """False: status 2."""
        if S.size < 2:
            return False
        x = self.t[S] - self.t[S[0]]
        y = self.D[S]
        n = float(S.size)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = (n * (x * y).sum() - x.sum() * y.sum()) / (n * (x * x).sum() - x.sum() ** 2)
        if not (math.isfinite(a) and a < 0.0):
            return False
        c = (y.sum() - a * x.sum()) / n
        self.a = float(a)
        self.cross = float(self.t[S[0]] + (self.V - c) / a)
        return True

    def search(self):
        """The eight numbers of the row."""
        p = self.p
        E = self.at(self.o) if self.n1 > 0 else 0.0
        bad = lambda status, knee=NAN: [E, NAN, knee, NAN, NAN, NAN, NAN, float(status)]
        if self.cap < 1 or not E > 0.0:
            return bad(1)
        w0 = min(p["window"] or int(math.floor(0.03 * self.rate + 0.5)), self.cap)
        if not self.noise(self.N - self.tail):
            return bad(3, float(self.N))
        self.means(w0)
        if not self.fit(self.run(False)):
            return bad(2)
        tc = self.cross
        arg = -10.0 / (self.a * p["per_decade"]) + 0.5
        self.margins["interval"].append(abs(arg - round(arg)))
        w = int(min(max(math.floor(arg), 1.0), float(self.cap)))
        self.means(w)
        prev = tc
        for _ in range(p["rounds"]):
            arg = tc + p["margin_db"] / -self.a
            self.margins["ceil"].append(abs(arg - round(arg)) if abs(arg) < 2.0 ** 52 else math.inf)
            a_n = int(min(max(math.ceil(arg), float(self.o)), float(self.N - self.tail)))
            if not self.noise(a_n):
                return bad(3, float(self.N))
            if not self.fit(self.run(True)):
                return bad(2)
            prev, tc = tc, self.cross
        with np.errstate(divide="ignore"):
            ptn = 10.0 * math.log10(float(self.P.max()) / self.Nz)
        return [E, self.Nz, tc, -60.0 / (self.a * float(self.rate)), ptn, float(w), abs(tc - prev), 0.0]


def floor(taps, rate, xovers=(), onset_db=-20.0, end=0, **kw):
    """taps: float32 [n, 2] as Convolution.ir_taps gives them.  Returns what Convolution.ir_floor returns, plus "margins":
    {(group, set): {decision: [distances]}}."""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    p = dict(DEFAULTS, **kw)
    for k in ("tail_fraction", "margin_db", "span_db"):
        p[k] = _f32(p[k])
    taps = np.asarray(taps, np.float32).reshape(-1, 2)
    n = taps.shape[0]
    N = min(int(end), n) if end else n
    o = ir_decay_np.origin(taps, N, _f32(onset_db))
    x = taps[:N].astype(np.float64)
    rows, margins = {}, {}
    for g, y in enumerate(groups_of(x, tuple(xovers), rate)):
        edc = edc_of(y, o)
        for s, name in enumerate(SETS):
            r = _Row(edc[s], o, N, rate, p)
            rows[(g, name)] = dict(zip(FIELDS, r.search()))
            margins[(g, name)] = r.margins
    return dict(origin=o, taps=N, rows=rows, margins=margins, query=dict(p, rate=rate, xovers=tuple(xovers), onset_db=onset_db, end=end))


def smallest_margin(res):
    return min((v for m in res["margins"].values() for vals in m.values() for v in vals), default=math.inf)


def assert_margins(res, least=1e-9):
    """What every comparison with the device asserts on the restatement first: no interval level within 1e-9 dB of a threshold,
    the two largest interval means 1e-9 dB apart, the interval's rounding 1e-9 from .5 and every ceil's argument 1e-9 from an
    integer, so that a discrete decision falling the other way cannot pass for an arithmetic difference."""
    for key, m in res["margins"].items():
        for what, vals in m.items():
            for v in vals:
                assert v > least, (key, what, v)


def check_against(got, want, rel=1e-6):
    """got: Convolution.ir_floor's result; want: floor()'s.  Status and interval equal exactly, NaN where and only where the
    restatement has NaN; energy, noise and T within 1e-6 relative; the knee within 1e-6 of its distance from the origin and the
    last change within the same bound; peak-to-noise within 1e-6 dB.  Prints the largest differences."""
    assert got["origin"] == want["origin"] and got["taps"] == want["taps"], (got["origin"], got["taps"], want["origin"], want["taps"])
    assert set(got["rows"]) == set(want["rows"])
    worst = dict.fromkeys(FIELDS, 0.0)
    for key, w in want["rows"].items():
        g = got["rows"][key]
        assert g["status"] == w["status"], (key, g, w)
        for f in FIELDS:
            assert np.isnan(g[f]) == np.isnan(w[f]), (key, f, g[f], w[f])
            if np.isnan(w[f]):
                continue
            if f in ("interval", "status") or np.isinf(w[f]):
                assert g[f] == w[f], (key, f, g[f], w[f])
                continue
            if f in ("knee", "last_change"):
                scale = max(abs(w["knee"] - want["origin"]), 1.0)
                err = abs(g[f] - w[f]) / scale
            elif f == "peak_to_noise_db":
                err = abs(g[f] - w[f])
            else:
                err = abs(g[f] - w[f]) / abs(w[f]) if w[f] else abs(g[f])
            worst[f] = max(worst[f], err)
    print("largest differences:", ", ".join(f"{f} {v:.1e}" for f, v in worst.items()))
    for f, v in worst.items():
        assert v <= rel, (f, v)


def noisy_ir(n=6000, lead=37, rate=8000, t60=0.25, floor_db=-50.0, seed=7, noise_seed=101):
    """ir_decay_np.noise_ir plus stationary Gaussian noise of amplitude 0.3 * 10^(floor_db / 20) in both channels of every frame
    after the lead, float32; its analytic crossing is lead + (-floor_db / 60) t60 rate."""
    ir = ir_decay_np.noise_ir(n, lead, rate, t60, seed=seed).astype(np.float64)
    rng = np.random.default_rng(noise_seed)
    ir[lead:] += 0.3 * 10.0 ** (floor_db / 20.0) * rng.standard_normal((n, 2))
    return ir.astype(np.float32)


def tail_from_floor(res, first=0):
    """The fields mc_ir_tail_from_floor fills, from a floor() result: dict(xovers, knee, t60, level_db) with knee None for a band
    that is left alone."""
    q = res["query"]
    rate, X = q["rate"], len(q["xovers"])
    knee, t60, level = [], [], []
    for j in range(X + 1):
        g = j + 1 if X else 0
        lr = res["rows"][(g, "LR")]
        if lr["status"] != 0 or not math.isfinite(lr["knee"]) or math.floor(lr["knee"]) >= res["taps"]:
            knee.append(None), t60.append(1), level.append((0.0, 0.0))
            continue
        k = int(math.floor(lr["knee"]))
        knee.append(first + k)
        t60.append(max(1, int(math.floor(lr["t"] * rate + 0.5))))
        lv = []
        for name in ("L", "R"):
            r = res["rows"][(g, name)]
            if r["status"] == 0:
                lv.append(10.0 * math.log10(r["noise"]) + (-60.0 / (r["t"] * rate)) * (k - r["knee"]))
            else:  # (the channel has no line of its own: half of what the pair has)
                lv.append(10.0 * math.log10(lr["noise"]) + (-60.0 / (lr["t"] * rate)) * (k - lr["knee"]) - 10.0 * math.log10(2.0))
            lv[-1] = _f32(lv[-1])
        level.append(tuple(lv))
    return dict(xovers=q["xovers"], knee=knee, t60=t60, level_db=level)
