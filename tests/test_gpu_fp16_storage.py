"""fp16 storage (mc_config.precision = 1) against a restatement that rounds as the engine does (tests/fp16_np.py).

A  the stored halves of every IR are the rounding of its fp32 spectra under the scale rule, bit for bit;
B  the delay line's fp16 mirror is the rounding of the fp32 delay line, bit for bit, whoever wrote the slots;
C  the partition sums: the engine's output against the float64 restatement fed the engine's own fp32 buffers, quantised,
   within a bar measured on an fp32 engine in the same test (4 x its own distance to the unquantised restatement, and
   never more than 1e-4 of the wet RMS);
D  the same through the instantiation that reads a gain per slot (a select fading over 100 blocks);
E  in C and D the fp16 engine's output differs from the fp32 engine's by more than 100 x the bar: the reduced path ran;
F  an IR whose largest tap is 1e-36 (its scale would overflow without the clamp of load_ir).
The inputs are fp16_np's; tests/test_fp16_np_cpu.py shows on the same inputs that every fault these tests are for moves the
restated output by more than ten times the ceiling."""
import numpy as np
import pytest

import fp16_np as f16

pytestmark = pytest.mark.gpu

CEILING = 1e-4
E32_MAX = 1e-5
MAXB = 64
WINDOW = {"a": 64, "b": 64, "c": 16, "d": 8, "e": 64}  # blocks of the last batch that are compared (the restatement's cost grows with P)
PERIOD_WINDOW = 16


def _engine(n_ref, prec, irs, period=256, max_batch=MAXB, sample_rate=None, wet=1.0):
    from cuda_audio_amd.engine import Convolution

    c = Convolution("fp16", n_ref, max_batch=max_batch, compat=False, precision=prec, period=period, sample_rate=sample_rate)
    for i, ir in enumerate(irs):
        c.prepare(i, ir)
    for h in (0, 1):
        c.cc[h].value.update(select=min(h, len(irs) - 1), dry=0.0, wet=wet, level=1.0, panWet=0.0, vsteps=0)
    return c


def _ring_of(n_ref):
    """The delay line's slots of an engine of this shape (the same in either precision)."""
    c = _engine(n_ref, "fp16", [f16.flat_ir(300, 1)])
    ring = c.debug_dims()["ring"]
    c.close()
    return ring


def _batches(c, x, b0, nb, size=MAXB):
    """Blocks b0 .. b0 + nb - 1 of x in batches of `size`; returns the outputs [2][256 nb]."""
    out = np.zeros((2, nb * 256), np.float32)
    b = b0
    while b < b0 + nb:
        n = min(size, b0 + nb - b)
        out[:, (b - b0) * 256:(b - b0 + n) * 256] = c.process(x[0, b * 256:(b + n) * 256], x[1, b * 256:(b + n) * 256])
        b += n
    return out


def _periods(c, x, b0, nb, pm):
    out = np.zeros((2, nb * 256), np.float32)
    for b in range(b0, b0 + nb, pm):
        s = slice(b * 256, (b + pm) * 256)
        o = slice((b - b0) * 256, (b - b0 + pm) * 256)
        out[0, o], out[1, o] = c.onProcess(x[0, s], x[1, s])
    return out


def _no_inf_nan(bits):
    return not np.any((bits & 0x7C00) == 0x7C00)


def _check_stored(c, idx):
    """A: the halves of IR idx are its fp32 spectra under the scale rule, over all 256 x pstride entries."""
    H32 = c.ir_spectra32(idx)
    scale = f16.scale_rule(H32)
    assert c.ir_scale16(idx) == scale
    bits = c.ir_spectra16(idx)
    assert bits.shape == H32.shape
    assert _no_inf_nan(bits)
    assert np.array_equal(bits, f16.quantise(H32, scale))
    return H32, bits


# ---- A

@pytest.mark.parametrize("tier", list(f16.TIERS))
def test_stored_spectra_are_the_rounded_fp32_spectra(gpu_lib, tier):
    irs = f16.tier_irs(tier) + [f16.wide_ir()]
    c = _engine(f16.TIERS[tier][0], "fp16", irs)
    scales = []
    for i in range(3):
        H32, bits = _check_stored(c, i)
        scales.append(c.ir_scale16(i))
        P = (len(irs[i]) + 255) // 256
        assert not np.any(bits[:, P:] & 0x7FFF)  # the padding beyond P is zero
    assert scales[0] > scales[1]  # IR 1 is 64 times louder
    Hw, bw = _check_stored(c, 2)
    sub = ((bw & 0x7C00) == 0) & ((bw & 0x03FF) != 0)
    assert sub[:, 3].mean() > 0.9  # the wide IR: its quietest partition is stored as subnormal halves
    assert sub[:, 2].mean() < 0.5 and np.mean((bw[:, 2] & 0x7FFF) != 0) > 0.99  # ... the one at 1e-7 mostly as normal ones
    c.close()


def test_stored_spectra_after_reloads_and_a_shaped_converted_load(gpu_lib):
    from cuda_audio_amd.engine import IrShape

    long_ir, short_ir = f16.flat_ir(7000, 1), f16.flat_ir(900, 2, 37.0)
    c = _engine(8192, "fp16", [long_ir, long_ir], sample_rate=48000)
    _check_stored(c, 0)
    c.prepare(0, short_ir)  # a shorter IR over a longer one: nothing of the longer one's halves may stay
    H32, bits = _check_stored(c, 0)
    assert not np.any(bits[:, 4:] & 0x7FFF) and not np.any(H32[:, 4:])
    c.prepare(1, f16.flat_ir(5000, 3, 5.0), ir_rate=44100, shape=IrShape(reverse=True, fade_out=512, normalize="peak", target=0.3))
    _check_stored(c, 1)
    c.close()


def test_stored_spectra_of_merged_entries(gpu_lib):
    """More IRs cross-fading in a half than there are voices (as test_more_irs_crossfading_than_voices forces it), on an fp16
    engine: every merged entry's halves are the rounding of its own fp32 spectra under its own scale, and no half overflows.
    The scale comes from a bound on the sources, B = sum_j |c_j| 2^14 / scale16_j >= max |M| (fp16_np.scale_rule_merged, checked
    on the CPU); the coefficients c_j cannot be read, so the rule is held from both sides instead.  It is never larger than the
    rule on the entry's own spectra.  After a half's FIRST merge, whose sources are loaded IRs, it is at most 2^4 smaller:
    2^14 / scale16_j <= 4 max |H_j|; the entries of M = sum c_j H_j, independent noise spectra, are as spread as
    sqrt(sum c_j^2 s_j^2) >= sum |c_j| s_j / sqrt(3) for three sources of spreads s_j, and its largest entry stands as far above
    that spread as each source's does above its own, give or take a third; so B / max |M| <= 4 sqrt(3) 1.3 = 9 < 2^4 (frexp
    rounds B up to the next power of two, which the rule does to max |M| as well).  A later merge takes the earlier merged
    entry as a source, with ITS bound for a maximum, so the distance compounds (measured over this sweep: 2^2 to 2^6); there
    only the upper side and the bits are held, and the distances are printed."""
    import ctypes as C

    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import Convolution
    from cuda_audio_amd.synth import make_input, make_ir

    nb, n_ref, first_merges = 100, 8192, 28
    x = make_input(nb * 256)
    c = Convolution("merge", n_ref, max_batch=16, precision="fp16")
    for j in range(7):
        c.prepare(j, make_ir(3000 + 450 * j, seed=60 + j, norm=0.05 * 4.0 ** (j % 3)))
    cmap = (21, 22, 23, 24, 25, 26, 27, 28)
    arr = (C.c_uint8 * 8)(*cmap)
    # half 0 takes its fourth IR at block 20 and its fifth, which fits beside the merged one, at 25; half 1 its fourth at 22:
    # at block 28 each half has merged exactly once.  Then the sweep goes on and the halves merge again and again
    events = {0: [(0, 25, 13), (1, 25, 13), (0, 22, 5)], first_merges: []}
    for k, sel in enumerate([1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1, 0]):
        events.setdefault(10 + 5 * k, []).append((0, 21, int(np.ceil(sel * 128 / 7))))
    for q, sel in zip([12, 17, 22, 40, 49, 58, 67], [3, 6, 1, 4, 0, 5, 2]):
        events.setdefault(q, []).append((1, 21, int(np.ceil(sel * 128 / 7))))

    def entries(single_level):
        allocated = []
        for idx in range(256, 260):
            try:
                H32 = c.ir_spectra32(idx)
            except McError as err:
                assert err.code == -1, err  # MC_ERR_ARG: never allocated, like an unloaded IR; nothing else is expected here
                for read in (c.ir_spectra16, c.ir_scale16):
                    with pytest.raises(McError):
                        read(idx)
                continue
            allocated.append(idx)
            scale, rule = c.ir_scale16(idx), f16.scale_rule(H32)
            bits = c.ir_spectra16(idx)
            print(f"merged entry {idx} after {'one merge' if single_level else 'the sweep'}: scale16 2^{int(np.log2(scale))}, "
                  f"the rule on its own spectra 2^{int(np.log2(rule))}")
            assert _no_inf_nan(bits)
            assert np.frexp(scale)[0] == 0.5 and 0 < scale <= rule
            if single_level:
                assert scale >= rule / 16
            assert np.array_equal(bits, f16.quantise(H32, scale))
        return allocated

    q = 0
    while q < nb:
        if q == first_merges:
            # a half's first merge goes to its second buffer (consolidate_voices: buf = 1 - mix_buf[i], entry 256 + 2 i + buf)
            assert entries(True) == [257, 259]
        for half, ctl, val in events.get(q, []):
            assert c._L.mc_handle_cc(c._h, half, arr, ctl, val) == 0
        n = min(16, min([e for e in events if e > q] + [nb]) - q)
        y = c.process(x[0, q * 256:(q + n) * 256], x[1, q * 256:(q + n) * 256])
        assert np.all(np.isfinite(y))
        q += n
    assert entries(False) == [256, 257, 258, 259]  # ... and the next ones to the first
    with pytest.raises(McError):
        c.ir_spectra16(7)  # an unloaded IR
    c.close()


def test_fp16_items_refuse_an_fp32_engine(gpu_lib):
    from cuda_audio_amd._lib import McError

    c = _engine(8192, "fp32", [f16.flat_ir(3000, 1)])
    for read in (lambda: c.ir_spectra16(0), lambda: c.ir_scale16(0), c.delay_line16):
        with pytest.raises(McError):
            read()
    assert c.slot_gains().shape[0] == 3 and c.delay_line().shape[0] == 256  # readable on either precision
    c.close()


# ---- B

def _mirror_ok(c):
    X = c.delay_line()
    assert np.array_equal(c.delay_line16(), f16.quantise(X, f16.FDL16_SCALE))
    return X


@pytest.mark.parametrize("tier", ["a", "b"])
def test_mirror_is_the_rounded_delay_line(gpu_lib, monkeypatch, tier):
    n_ref = f16.TIERS[tier][0]
    irs = f16.tier_irs(tier)
    # batches that wrap the ring at least twice, of a length that leaves partial tiles; then a mix with periods; then reset
    c = _engine(n_ref, "fp16", irs)
    ring = c.debug_dims()["ring"]
    nb = 2 * ring + 100
    x = f16.stream("noise", (nb + 64) * 256)
    _batches(c, x, 0, nb, size=37)
    X = _mirror_ok(c)
    assert np.all(np.any(X != 0, axis=(0, 2)))  # every slot of the ring has been written
    b = nb
    for n, how in ((5, "p"), (23, "b"), (3, "p"), (8, "b"), (1, "p")):
        (_periods(c, x, b, n, 1) if how == "p" else _batches(c, x, b, n))
        b += n
    _mirror_ok(c)
    c.reset()
    assert not np.any(c.delay_line()) and not np.any(c.delay_line16())
    c.close()
    # 256-frame periods in both forms of partition 0
    for form, key in (("fd", "frequency_domain"), ("td", "time_domain")):
        monkeypatch.setenv("MCCONV_TAIL_FORM", form)
        c = _engine(n_ref, "fp16", irs)
        _periods(c, x, 0, 40, 1)
        forms = c.tail_forms()
        assert forms[key] > 0 and sum(forms.values()) == forms[key], forms
        X = _mirror_ok(c)
        assert np.all(np.any(X[:, :40] != 0, axis=(0, 2)))
        c.close()
    monkeypatch.delenv("MCCONV_TAIL_FORM")
    # 512- and 1024-frame periods
    for period in (512, 1024):
        pm = period // 256
        c = _engine(n_ref, "fp16", irs, period=period)
        _periods(c, x, 0, 40, pm)
        X = _mirror_ok(c)
        assert np.all(np.any(X[:, :40] != 0, axis=(0, 2)))
        c.close()


# ---- C, D, E, F

class _State:
    """An engine's own buffers after a run: what the restatement is fed."""

    def __init__(self, c, nirs=2):
        self.H = [c.ir_spectra32(i) for i in range(nirs)]
        self.X = c.delay_line()
        self.G = c.slot_gains()
        self.ring = self.X.shape[1]

    def quantised(self):
        self.sc = [f16.scale_rule(h) for h in self.H]
        self.Hq = [f16.dequantise(f16.quantise(h, s)) for h, s in zip(self.H, self.sc)]
        self.Xq = f16.dequantise(f16.quantise(self.X, f16.FDL16_SCALE))

    def wet(self, first, n, hi, voices, lo16=None):
        """Blocks first .. first + n - 1, restated; lo16 = None: unquantised."""
        slots = np.arange(first - 1, first + n)
        Y = 0.0
        for v, i0, i1 in voices:
            if lo16 is None:
                Y = Y + f16.partition_sum(self.H[i0], self.H[i1], self.X, self.G[v], slots, 0, hi)
            else:
                Y = Y + f16.partition_sum_q(self.H[i0], self.H[i1], self.X, self.Hq[i0], self.Hq[i1], self.Xq, self.sc[i0], self.sc[i1],
                                            self.G[v], slots, lo16, hi)
        return f16.wet_blocks(Y)


def _steady_voices(st, first, n, hi):
    """Select h on half h from the first block on: whatever row carries gains carries IR 0 for input 1 and IR 1 for input 2."""
    reach = np.arange(first - 1 - hi, first + n) & (st.ring - 1)
    rows = [(v, 0, 1) for v in range(3) if np.any(st.G[v][reach])]
    assert rows
    return rows


def _slot_check(st, x, last):
    """The bookkeeping this file relies on: block t of the stream sits in slot t & (ring - 1)."""
    want = f16.spectra(x[:, last * 256:(last + 1) * 256].T)[:, 0]
    got = st.X[:, last & (st.ring - 1)]
    assert np.abs(got - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-30)


def _judge(label, got32, st32, got16, st16, first, n, hi, lo16, voices32, voices16):
    st16.quantised()
    e32 = f16.worst_block(got32, st32.wet(first, n, hi, voices32))
    e16 = f16.worst_block(got16, st16.wet(first, n, hi, voices16, lo16))
    diff = f16.worst_block(got16, got32)
    print(f"fp16-storage {label}: e32 {e32:.3e}  fp16 {e16:.3e}  fp16 against fp32 engine {diff:.3e}  (worst block / wet RMS)")
    assert np.all(np.isfinite(got16)) and np.all(np.isfinite(got32))
    assert max(np.abs(got16).max(), np.abs(got32).max()) < 0.9  # (inside the output's saturating clamp)
    assert e32 <= E32_MAX, (label, e32)
    assert e16 <= 4 * e32, (label, e16, e32)
    assert e16 <= CEILING, (label, e16)
    assert diff > 100 * min(4 * e32, CEILING), (label, diff, e32)  # E: the reduced path is the one that ran
    return e32, e16, diff


def _sum_case(tier, kind, path, irs=None, label=None, wrap=False, wet=1.0, form=None):
    """wrap: the compared window straddles the end of the ring on its second lap - block 2 ring sits in slot 0 - so the sweep's
    `(slot0 + t - p) & (ring - 1)` and the host's slot0 run across the wrap and every partition reaches back into slots that have
    been written over once.  Without it the run starts cold and ends well inside the first lap.
    form: 'td' / 'fd' - the form of partition 0 the 256-frame tails were forced to (MCCONV_TAIL_FORM, set by the caller)."""
    n_ref, taps = f16.TIERS[tier]
    irs = irs if irs is not None else f16.tier_irs(tier)
    P = (max(len(ir) for ir in irs) + 255) // 256
    hi = (P + 15) // 16 * 16
    ring = _ring_of(n_ref)
    assert ring > hi + MAXB
    got, st = {}, {}
    if path == "batch":
        n = WINDOW[tier]
        # at least P + 64 blocks, then the batch that is compared
        lead = 2 * ring - MAXB // 2 if wrap else (P + 64 + MAXB - 1) // MAXB * MAXB
        nb = lead + MAXB
        x = f16.stream(kind, nb * 256)
        first = nb - n
        for prec in ("fp32", "fp16"):
            c = _engine(n_ref, prec, irs, wet=wet)
            _batches(c, x, 0, lead)
            got[prec] = _batches(c, x, lead, MAXB)[:, (MAXB - n) * 256:]
            st[prec] = _State(c)
            c.close()
    else:
        pm = path // 256
        n = PERIOD_WINDOW
        nper = 2 * n
        # by batches; then periods, the last n blocks of which are compared
        lead = 2 * ring - nper + n // 2 if wrap else (P + 64 + MAXB - 1) // MAXB * MAXB
        nb = lead + nper
        x = f16.stream(kind, nb * 256)
        first = nb - n
        for prec in ("fp32", "fp16"):
            c = _engine(n_ref, prec, irs, period=path, wet=wet)
            _batches(c, x, 0, lead)
            got[prec] = _periods(c, x, lead, nper, pm)[:, (nper - n) * 256:]
            if form and prec == "fp16":
                forms = c.tail_forms()
                key = dict(td="time_domain", fd="frequency_domain")[form]
                assert forms[key] > 0 and sum(forms.values()) == forms[key], forms
            st[prec] = _State(c)
            c.close()
    if wrap:
        assert first < 2 * ring < first + n and st["fp16"].ring == ring
    for prec in got:
        _slot_check(st[prec], x, nb - 1)
    label = label or f"tier {tier} {path} {kind}" + (", across the ring's end" if wrap else "") + (f", partition 0 forced {form}" if form else "")
    return _judge(label, got["fp32"], st["fp32"], got["fp16"], st["fp16"], first, n, hi, f16.LO16[path],
                  _steady_voices(st["fp32"], first, n, hi), _steady_voices(st["fp16"], first, n, hi))


@pytest.mark.parametrize("tier,kind", [("a", "noise"), ("a", "full"), ("a", "quiet"), ("b", "noise"), ("c", "noise"), ("d", "noise"),
                                       ("e", "noise")])
def test_batch_sum_matches_the_quantised_restatement(gpu_lib, tier, kind):
    _sum_case(tier, kind, "batch")


@pytest.mark.parametrize("tier,kind", [("a", "noise"), ("a", "quiet"), ("b", "noise"), ("e", "noise")])
def test_batch_sum_across_the_rings_end(gpu_lib, tier, kind):
    _sum_case(tier, kind, "batch", wrap=True)


@pytest.mark.parametrize("period", [256, 512, 1024])
@pytest.mark.parametrize("tier,kind", [("a", "noise"), ("a", "quiet"), ("b", "noise"), ("e", "noise")])
def test_period_sum_matches_the_quantised_restatement(gpu_lib, tier, kind, period):
    _sum_case(tier, kind, period)


@pytest.mark.parametrize("period", [256, 512, 1024])
@pytest.mark.parametrize("tier,kind", [("a", "noise"), ("a", "quiet"), ("b", "noise")])
def test_period_sum_across_the_rings_end(gpu_lib, tier, kind, period):
    _sum_case(tier, kind, period, wrap=True)


@pytest.mark.parametrize("form", ["td", "fd"])
@pytest.mark.parametrize("kind", ["noise", "quiet"])
def test_256_frame_period_sum_in_either_form_of_partition_0(gpu_lib, monkeypatch, kind, form):
    """The tail sums partition 0 in the frequency domain or, forced here, in the time domain against the IR's first 256 fp32 taps:
    neither reads a half, and one restatement (lo16 = 2) serves both."""
    monkeypatch.setenv("MCCONV_TAIL_FORM", form)
    _sum_case("a", kind, 256, wrap=True, form=form)


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("tier", ["a", "b"])
def test_fading_select_matches_the_quantised_restatement(gpu_lib, tier, wrap):
    """D: half 0 moves from IR 0 to IR 1 over 100 blocks; the batch inside the fade reads a gain per slot.  wrap: as in _sum_case."""
    n_ref, taps = f16.TIERS[tier]
    irs = f16.tier_irs(tier)
    P = (max(taps) + 255) // 256
    hi = (P + 15) // 16 * 16
    lead = 2 * _ring_of(n_ref) - MAXB // 2 if wrap else (P + 64 + MAXB - 1) // MAXB * MAXB
    nb = lead + MAXB
    x = f16.stream("noise", nb * 256)
    got, st, voices = {}, {}, {}
    for prec in ("fp32", "fp16"):
        c = _engine(n_ref, prec, irs)
        _batches(c, x, 0, lead)
        c.cc[0].value.update(select=1, vsteps=100)
        got[prec] = _batches(c, x, lead, MAXB)
        s = st[prec] = _State(c)
        c.close()
        # the rows: the one that sounded before the fade carries IR 0 (fading out) and half 1's IR 1; the new one IR 1 for input 1
        before, newest = (lead - 1) & (s.ring - 1), (nb - 1) & (s.ring - 1)
        old = [v for v in range(3) if np.any(s.G[v][before])]
        new = [v for v in range(3) if v not in old and np.any(s.G[v][newest])]
        assert len(old) == 1 and len(new) == 1, (old, new)
        fade = s.G[:, np.arange(lead, nb) & (s.ring - 1)]
        assert len(np.unique(fade[old[0], :, 0])) == MAXB and len(np.unique(fade[new[0], :, 0])) == MAXB  # a gain per slot
        assert np.all(np.diff(fade[old[0], :, 0]) < 0) and np.all(np.diff(fade[new[0], :, 0]) > 0)
        assert not np.any(fade[new[0]][:, [1, 3]])  # the new row carries nothing for input 2
        voices[prec] = [(old[0], 0, 1), (new[0], 1, 1)]
        _slot_check(s, x, nb - 1)
    _judge(f"tier {tier} batch fading select" + (", across the ring's end" if wrap else ""), got["fp32"], st["fp32"], got["fp16"], st["fp16"], lead, MAXB, hi, 0, voices["fp32"], voices["fp16"])


@pytest.mark.parametrize("wet,wrap", [(1.0, False), (0.3, True)])
def test_quiet_ir(gpu_lib, wet, wrap):
    """F: IRs whose largest taps are 1e-36 and 64e-36.  Without a clamp load_ir's scale 2^(13 - ex) is infinite for them.
    wet = 0.3: the inverse scale is 2^-126 here, so a gain below 1 times it is a subnormal float - the sum is right only while the
    device keeps fp32 subnormals, which fp16_np.inv_gains restates (numpy keeps them)."""
    irs = f16.tier_irs("a")
    irs = [(ir.astype(np.float64) * (1e-36 / np.abs(irs[0]).max())).astype(np.float32) for ir in irs]
    assert 0.9999e-36 <= np.abs(irs[0]).max() <= 1.0001e-36
    c = _engine(8192, "fp16", irs)
    for i in (0, 1):
        assert np.isfinite(c.ir_scale16(i)) and c.ir_scale16(i) > 0
        _check_stored(c, i)
    c.close()
    _sum_case("a", "noise", "batch", irs=irs, wet=wet, wrap=wrap,
              label=f"tier a batch noise, IRs at 1e-36, wet {wet}" + (", across the ring's end" if wrap else ""))
