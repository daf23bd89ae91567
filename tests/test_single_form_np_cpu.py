"""tests/single_form_np.py on the CPU: the accumulator layout is undone exactly, the error read-out points at the row or the
residue class that is wrong, and the numpy restatement whose accumulator the GPU tests read is the one the C oracle agrees with."""
import numpy as np
import pytest

from helpers import BASE
from single_form_np import ROW, acc_errors, acc_frames, flat_ir, oracle_run, ring_from_frames, white_input


@pytest.mark.parametrize("M", [8, 2048])
def test_acc_frames_undoes_the_ring_layout(M):
    """A ring built slot by slot from the layout formula of singlefft.hip.h (slot t = (base + s) mod N at
    [c][t mod 512][t / 512]) gives back the frame sequence it was built from, at every position of the origin."""
    N = ROW * M
    frames = np.stack([np.arange(N, dtype=np.float32), -np.arange(N, dtype=np.float32) - 0.5])  # every entry distinct, exact in fp32
    for base in (0, 256, 3 * 256, 512, N // 2 + 5 * 256, N - 256):
        raw = ring_from_frames(frames, N, base)
        assert raw.shape == (2 * N,)
        got = acc_frames(raw, N, base)
        assert got.shape == (2, N) and np.array_equal(got, frames), base
        for c, s in ((0, 0), (1, 1), (0, 255), (1, 256), (0, 511), (1, 512), (0, N - 257), (1, N - 1)):  # the formula, slot by slot
            t = (base + s) % N
            assert raw[c * N + (t % 512) * M + t // 512] == frames[c, s]
    # (a wrong origin is seen: the same ring read half a row off)
    assert not np.array_equal(acc_frames(ring_from_frames(frames, N, 256), N, 0), frames)


def test_acc_errors_points_at_the_row_and_at_the_class():
    N, M = 16384, 32
    rng = np.random.default_rng(3)
    want = rng.standard_normal((2, N)) * 0.05
    want[:, N - 1024:] = 0
    clean = acc_errors(want.astype(np.float32), want, lo=301, hi=N - 1024)
    assert clean["rms"] < 1e-8 and clean["worst_row"] < 1e-8 and clean["worst_class"] < 1e-8
    assert list(clean["live_rows"]) == list(range(1, 30))  # row 0 holds frames before 301, rows 30 and 31 the emptied end
    assert clean["row_rms"].shape == (M,) and clean["class_rms"].shape == (ROW,)
    assert clean["row_rms"][31] == 0 and clean["row_floor"] > 0.04 and clean["class_floor"] > 0.02
    assert clean["peak"] == np.abs(want).max()

    got = want.copy()
    got[1, 21 * ROW:22 * ROW] += 1e-3  # one row of one channel
    r = acc_errors(got, want)
    assert r["worst_row_at"] == 21
    assert r["worst_row"] == pytest.approx(1e-3 / np.sqrt(2), rel=1e-6)
    assert r["rms"] == pytest.approx(1e-3 / np.sqrt(2 * M), rel=1e-6)  # diluted by the other rows
    assert r["worst_class"] == pytest.approx(r["rms"], rel=1e-6)  # every class carries one bad entry in M

    got = want.copy()
    got[0, 77::ROW] -= 1e-3  # one residue class
    r = acc_errors(got, want)
    assert r["worst_class_at"] == 77
    assert r["worst_class"] == pytest.approx(1e-3 / np.sqrt(2), rel=1e-6)
    assert r["worst_row"] == pytest.approx(1e-3 / np.sqrt(2 * ROW), rel=1e-6)

    # a quiet row or class inside the live range shows in the floors
    quiet = want.copy()
    quiet[:, 5 * ROW:6 * ROW] = 0
    assert acc_errors(quiet, quiet, lo=301, hi=N - 1024)["row_floor"] == 0
    quiet = want.copy()
    quiet[:, 300::ROW] = 0
    assert acc_errors(quiet, quiet, lo=301, hi=N - 1024)["class_floor"] == 0


def test_the_numpy_restatement_is_the_one_the_c_oracle_agrees_with(oracle_mod):
    """RefCompatNp (whose accumulator the GPU tests read) against oracle.RefCompat (which the single-form tests trust for the
    outputs): the same outputs to 1e-12 over calls with unequal halves, a predelay and an event; and the accumulator handed
    back is the one those outputs came from: its first period is what the next call emits when fed silence."""
    n_ref, period, ncalls = 4096, 256, 8
    irs = [flat_ir(n_ref - 1024, 1, 0.02), flat_ir(n_ref - 1024, 2, 0.02)]
    x = white_input((ncalls + 1) * period, 4)
    x[:, ncalls * period:] = 0
    ev = {0: ((0, dict(BASE, select=0, predelay=301, wet=0.6, panWet=0.3, panDry=-0.2)), (1, dict(BASE, select=1, wet=0.4, level=0.8, panWet=-0.5, dry=0.3))),
          5: ((0, dict(predelay=0)), (1, dict(select=0, vsteps=3, speed=3)))}
    want_all, _ = oracle_run(n_ref, irs, x, ev, period)
    got, acc = oracle_run(n_ref, irs, x[:, :ncalls * period], ev, period)
    r = oracle_mod.RefCompat(n_ref, True)
    for i, ir in enumerate(irs):
        r.prepare(i, ir)
    ref = np.zeros_like(got)
    for q in range(ncalls):
        for half, p in ev.get(q, ()):
            r.set(half, **p)
        s = slice(q * period, (q + 1) * period)
        ref[:, s] = r.process(x[0, s], x[1, s], period)
    r.close()
    assert np.abs(ref).max() > 0.05
    assert np.abs(got - ref).max() <= 1e-12
    assert acc.shape == (2, n_ref) and np.all(acc[:, n_ref - period:] == 0)
    # the silent call adds a contribution of its own (the live spectra are there, the input is null: nothing) and emits acc[0:period]
    assert np.abs(want_all[:, ncalls * period:] - acc[:, :period]).max() <= 1e-12
