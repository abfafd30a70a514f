"""The engineered tracker sequences (tests/tracking_cases.py) on the CPU: the reference run of every case satisfies the
case's claim — written-down luts, slots, uids and dropped counts — and every mutant of the decision rules comes out
differently on each case named for it.  No GPU: tests/test_tracking_cases_gpu.py runs the same frames on the device."""
import numpy as np
import pytest

from tests import tracking_cases as TC
from tests.tracking_reference import ReferenceTracker


@pytest.fixture(scope="module")
def true_runs():
    return {name: TC.run_case(make())[0] for name, make in TC.CASES.items()}


def same(a, b):
    """out, lut, table, mem and meta of every step."""
    return len(a) == len(b) and all(all(np.array_equal(x, y) for x, y in zip(sa[:4], sb[:4])) and sa[4] == sb[4]
                                    for sa, sb in zip(a, b))


@pytest.mark.parametrize("name", list(TC.CASES))
def test_reference_run_satisfies_the_claim(true_runs, name):
    c = TC.CASES[name]()
    assert c["frames"].dtype == np.int32 and c["frames"].ndim == 3 and callable(c["claim"])
    c["claim"](true_runs[name])
    assert all(s[0].max() <= 127 for s in true_runs[name])


def test_every_issue_case_is_there():
    for name in ("tie_domino", "tie_larger_inter_many", "tie_lower_id_high", "threshold_equal_small", "threshold_equal_large",
                 "products_need_64_bits", "births_across_waves", "births_overflow", "junk_and_edges"):
        assert name in TC.CASES
    assert sum(n.startswith("tiny_") for n in TC.CASES) == 3
    assert set(TC.MOVED) | set(TC.ENGINEERED) == set(TC.CASES)


def test_the_domino_is_one_tie_over_the_whole_wave():
    c = TC.tie_domino()
    ref = ReferenceTracker(c["min_iou"], c["max_age"])
    ref.step(c["frames"][0])
    mem, cur = ref.mem.reshape(-1), c["frames"][1].reshape(-1)
    pairs = {}
    for t, i in zip(mem, cur):
        if t and i:
            pairs[(int(t), int(i))] = pairs.get((int(t), int(i)), 0) + 1
    assert len(pairs) == 252 > 64 and set(pairs.values()) == {2}                      # every intersection is 2 ...
    assert all((mem == t).sum() == 4 for t, _ in pairs) and all((cur == i).sum() == 4 for _, i in pairs)   # ... of 4 + 4 - 2
    assert min(t for t, _ in pairs) == 1 and max(t for t, _ in pairs) == 127
    assert min(i for _, i in pairs) < 64 < max(i for _, i in pairs)
    ref.step(c["frames"][1])
    assert ref.events["match"] == 126 and ref.events["birth"] == 0


def test_products_do_not_fit_32_bits():
    c = TC.products_need_64_bits()
    T, a, e5, e9 = (TC.P64[k] for k in ("T", "a", "e5", "e9"))
    f = c["frames"]
    assert f.shape[2] % 4 == 0 and f.shape[2] - (T + e5 + e9) < 4 and (f[0] == 1).sum() == T
    assert (f[1] == 5).sum() == a + e5 and (f[1] == 9).sum() == T - a + e9
    assert ((f[0] == 1) & (f[1] == 5)).sum() == a and ((f[0] == 1) & (f[1] == 9)).sum() == T - a
    assert a * (T + e9) < (T - a) * (T + e5) and (a * (T + e9)) % 2 ** 32 > ((T - a) * (T + e5)) % 2 ** 32


def test_births_cross_the_wave_boundary():
    for c, step, gone in ((TC.births_across_waves(), 1, TC.GONE), (TC.births_overflow(), 2, TC.GONE_FIRST)):
        run, ref = TC.run_case(c)
        before, after = run[step - 1][2], run[step][2]
        freed = [s for s in range(1, 128) if before[s, 0] and before[s, 0] != after[s, 0]]
        assert freed == list(gone) and min(freed) < 64 <= max(freed)                  # retired and reborn in one step
        new = [i for i in range(1, 128) if run[step][1][i] in gone]
        assert min(new) < 64 <= max(new) and sum(i < 64 for i in new) != sum(s < 64 for s in freed)   # the wave-1 offsets differ
        assert ref.events["reuse"] == len(gone) and ref.events["retire"] == len(gone)
    assert c["frames"].shape[0] == 3 and run[2][4]["dropped"] == 7


@pytest.mark.parametrize("rule", list(TC.MUTANTS))
def test_every_mutant_is_caught_by_the_cases_named_for_it(true_runs, rule):
    assert TC.MUTANTS[rule]
    for name in TC.MUTANTS[rule]:
        wrong, _ = TC.run_case(TC.CASES[name](), TC.MutantTracker, rule=rule)
        assert not same(wrong, true_runs[name]), f"{name} cannot tell '{rule}' from the true rule"
        with pytest.raises(AssertionError):
            TC.CASES[name]()["claim"](wrong)                                          # and the written-down answer says so


def test_the_mutants_are_the_eight_rules():
    with pytest.raises(AssertionError):
        TC.MutantTracker(rule="no such rule")
    assert len(TC.MUTANTS) == 8
