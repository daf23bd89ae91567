"""The cases of group_history_cases.py cannot pass by accident: in every window block the Q1/Q2 terms are worth at least
ten times the parity tolerance, so a rank that finishes such a block from a stale history misses the oracle.  A condition on
the inputs, shown with the float64 oracle; no GPU."""
import numpy as np
import pytest

import group_history_cases as ghc
from helpers import RMS_TOL

PERIOD_256 = [n for n, c in ghc.CASES.items() if c.period == 256]


def test_case_table_is_what_the_gpu_tests_assume():
    for name, c in ghc.CASES.items():
        pm = c.period // 256
        assert all(1 <= n <= ghc.MAX_BATCH and n % pm == 0 for n in c.sizes), name
        for ranks in c.ranks:
            ragged = [i for _, n, i in ghc.batches(c) if ghc.is_ragged(c, n, ranks)]
            assert ragged and ragged[-1] < len(c.sizes) - 1, f"{name}: an even batch must follow the last ragged one"
            win = ghc.window_blocks(c, ranks)
            assert win and win[-1] < sum(c.sizes)
            # some window block is finished by a rank >= 1 (that is where a missing history shows)
            assert max(ghc.finisher(c, ranks, b)[1] for b in win) >= 1, name
    assert ghc.window_blocks(ghc.CASES["ragged_then_even"], 2) == list(range(101, 101 + 64 + 2))
    assert ghc.window_blocks(ghc.CASES["ragged_first"]) == list(range(37, 101))
    assert ghc.window_blocks(ghc.CASES["tail_drop"]) == list(range(101, 165))  # (64 + 8 blocks, cut at the end of the run)
    assert ghc.finisher(ghc.CASES["ragged_then_even"], 4, 64 + 36) == (1, 0)
    assert ghc.finisher(ghc.CASES["ragged_then_even"], 4, 101 + 16) == (2, 1)
    assert ghc.finisher(ghc.CASES["period_512"], 4, 102 + 63) == (2, 3)


@pytest.mark.parametrize("name", PERIOD_256)
def test_window_blocks_depend_on_the_history(oracle_mod, name):
    case = ghc.CASES[name]
    x, want, win = ghc.build(oracle_mod, name)
    assert not x.flags.writeable and not want.flags.writeable
    assert want.shape == x.shape and np.abs(want).max() < 0.5  # nothing near the clamp
    win = np.asarray(win)
    for pd in sorted({case.predelay, *case.changes.values()}):  # (the partitioned oracle models one predelay per run: each in turn)
        share = ghc.compat_share(oracle_mod, name, pd)
        worst = int(win[np.argmin(share[win])])
        print(f"{name} predelay {pd}: compat share over the window blocks {share[win].min():.3e} .. {share[win].max():.3e}")
        assert share[worst] >= 10 * RMS_TOL, f"{name} predelay {pd}: block {worst} carries only {share[worst]:.3e}"


def test_the_two_oracles_agree_outside_the_q8_regime_and_part_inside_it(oracle_mod):
    """predelay_change, period_512 and tail_drop are judged by the single-transform restatement, the others by the partitioned
    oracle: the same samples where both apply.  In the Q8 regime they part: the partitioned oracle's state machine cuts the Q1/Q2
    windows at n_ref but keeps the wet tail the reference drops there (oracle.c, orc_upols_finish), which is worth more than the
    parity tolerance in tail_drop's window blocks - so that case takes the restatement, as the Q8 tests of test_gpu_parity.py do."""
    _, want, _ = ghc.build(oracle_mod, "ragged_first")
    assert ghc.block_rms(ghc._refcompat(oracle_mod, ghc.CASES["ragged_first"]) - want).max() <= 1e-12
    _, want, win = ghc.build(oracle_mod, "tail_drop")
    apart = ghc.block_rms(ghc._upols(oracle_mod, ghc.CASES["tail_drop"], True) - want)
    assert apart[:64].max() <= 1e-12 and apart[list(win)].max() > RMS_TOL
