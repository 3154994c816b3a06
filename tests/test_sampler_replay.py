"""The sampler's noise stream replayed on the host (tests/_sampler_cases.py): the two hash implementations agree,
the uniform is sound for every hash value, the stream samples softmax(x / T), the acceptance rule notices subtly
wrong samplers, the GPU cases hold few near-ties, and the CPU backend follows the replay."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_cases as sc  # noqa: E402

from chronos.ops import reference as ref  # noqa: E402


def test_the_two_hash_implementations_agree():
    tuples = sc.hash_tuples()
    assert 200 <= len(tuples) <= 1000
    for seed, nout, slot, v in tuples:
        h = ref.sampler_hash(seed, nout, slot, v + 1)
        assert int(h[v]) == sc.hash_int(seed, nout, slot, v), (seed, nout, slot, v)
        if v:
            assert int(h[v - 1]) == sc.hash_int(seed, nout, slot, v - 1)
    # the broadcast form (tensors of seeds / steps / slots) is the scalar form row by row
    s, n, b = (torch.tensor([t[i] for t in tuples[:64]]) for i in range(3))
    hb = ref.sampler_hash(s, n, b, 5)
    for i, (seed, nout, slot, _) in enumerate(tuples[:64]):
        assert hb[i].tolist() == [sc.hash_int(seed, nout, slot, v) for v in range(5)]


def test_the_uniform_is_sound_for_every_hash_value():
    h = np.arange(1 << (32 - sc.NEW_SHIFT), dtype=np.uint32)
    u = sc.uniform_np(h)
    assert sc.uniform_is_sound(u)
    assert float(u[0]) == 2.0 ** -24 and float(u[-1]) == 1.0 - 2.0 ** -24
    assert np.array_equal(u.astype(np.float64), (h.astype(np.float64) + 0.5) * 2.0 ** -23), "u is exact in fp32"
    # the reference forms the same bits from the unshifted hash (the low 9 bits do not matter)
    t = ref.uniform_of_hash(torch.from_numpy(h.astype(np.int64)) << sc.NEW_SHIFT | 0x1FF).numpy()
    assert t.dtype == np.float32 and np.array_equal(t, u)


def test_the_parents_uniform_fails_the_same_check():
    h = np.arange(1 << (32 - sc.OLD_SHIFT), dtype=np.uint32)
    u = sc.uniform_old_np(h)
    assert not sc.uniform_is_sound(u)
    assert float(u[-1]) == 1.0 and not bool((np.diff(u) > 0).all())
    for vocab, hits in sc.OLD_HITS.items():
        for seed, nout, slot, v in hits:
            assert v < vocab
            hs = sc.hash_int(seed, nout, slot, v) >> sc.OLD_SHIFT
            assert hs == (1 << 24) - 1 and float(sc.uniform_old_np(np.array([hs], dtype=np.uint32))[0]) == 1.0
            # the same token today: the largest u there is, below 1
            assert float(ref.sampler_uniform(seed, nout, slot, vocab)[v]) == 1.0 - 2.0 ** -24


def _chi2_quantile(dof, tail):
    """x with P(chi2_dof > x) = tail, by bisection on the regularised upper incomplete gamma function."""
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = (lo + hi) / 2
        q = float(torch.special.gammaincc(torch.tensor(dof / 2, dtype=torch.float64),
                                          torch.tensor(mid / 2, dtype=torch.float64)))
        lo, hi = (mid, hi) if q > tail else (lo, mid)
    return hi


DRAWS = 65536
SWEEPS = {"seed": lambda a: (a, 0, 0), "slot": lambda a: (0, 0, a), "nout": lambda a: (12345, a, 7)}


@pytest.mark.parametrize("sweep,T", [("seed", 0.5), ("seed", 1.0), ("seed", 2.0), ("slot", 1.0), ("nout", 1.0)])
def test_the_stream_samples_softmax(sweep, T):
    """65 536 Gumbel-max draws over six tokens against softmax(x / T): Pearson chi-square below the upper 1e-6
    quantile at 5 degrees of freedom.  The draws are fixed (consecutive seeds, slots or steps), so the statistic is a
    constant; a failure is a finding about the keying of mix32."""
    x = torch.tensor([2.0, 1.0, 0.5, 0.0, -1.0, -3.0], dtype=torch.float64)
    u = ref.sampler_uniform(*SWEEPS[sweep](torch.arange(DRAWS)), 6)
    assert u.shape == (DRAWS, 6) and u.dtype == torch.float32
    tok = (x / T - torch.log(-torch.log(u.double()))).argmax(1)
    obs = torch.bincount(tok, minlength=6).double()
    exp = torch.softmax(x / T, 0) * DRAWS
    stat = float(((obs - exp) ** 2 / exp).sum())
    bound = _chi2_quantile(5, 1e-6)
    print(f"chi-square over {sweep} at T = {T}: {stat:.2f} (bound {bound:.2f})")
    assert 35.0 < bound < 40.0
    assert stat < bound


@pytest.fixture(scope="module")
def wide():
    """4096 sampled rows of the first GPU case (V = 1003, no filter) at T = 1, with their fp64 replays."""
    c = sc.Case(1003, "bf16", n=4096, temps=(1.0,), all_live=True)
    slots = c.sampled()
    assert len(slots) == 4096
    return c, [c.scores(s) for s in slots]


@pytest.mark.parametrize("how", sc.MUTANTS)
def test_the_yardstick_notices_a_mutated_sampler(wide, how):
    c, scores = wide
    rejected = sum(not sc.judge(scores[s], sc.mutant_token(c, s, how), sc.G)[0] for s in range(c.n))
    print(f"mutant {how}: rejected in {rejected / c.n:.1%} of {c.n} rows at G = {sc.G}")
    assert rejected >= 0.01 * c.n


def test_the_yardstick_accepts_the_replay_itself(wide):
    c, scores = wide
    assert all(sc.judge(scores[s], sc.mutant_token(c, s, None), 0.0) == (True, 0.0) for s in range(0, c.n, 16))


@pytest.fixture(scope="module", params=sc.GPU_CASES, ids=sc.case_id)
def case(request):
    return sc.Case(**request.param)


def test_near_ties_are_rare_in_the_gpu_cases(case):
    slots = case.sampled()
    assert len(slots) >= 90
    near = sum(sc.top_two_gap(case.scores(s)) < sc.G for s in slots)
    print(f"{near} of {len(slots)} sampled rows have a top-two gap below G = {sc.G}")
    assert near <= 0.01 * len(slots)


def test_the_cpu_backend_follows_the_replay(case):
    """ops.constrained_sample on the CPU draws the device's stream: every sampled row gets the replay's argmax, and
    the whole slot state advances as the cases' own ``advance`` says."""
    before, after = case.run("cpu")
    gaps = []
    case.check_step(before, after, 0.0, gaps=gaps)
    assert not gaps
    kinds = {case.kinds[s] for s in range(case.n)}
    assert {"live", "done", "parked", "empty", "greedy", "neutral"} <= kinds
    closed = sum(int(after["state"][s]) == sc.DONE for s in case.sampled())
    parked = sum(int(after["state"][s]) < -1 for s in case.sampled())
    # every row that enters ST_NEAR parks when the jump table is given, none does without it
    assert parked == (len(case.sampled()) - closed if case.jump_c is not None else 0)
    assert closed > 0 or case.filt in ("topp", "both")  # a ladder's twenty tokens need not hold a closing one


def test_the_committed_g_is_derived_from_the_measured_gaps():
    rec = sc.load_gaps()
    largest = max(float(v["max_gap"]) for v in rec["cases"].values())
    assert largest <= sc.G_CAP, "a disagreement above 2^-7 is a failure, not a tolerance"
    assert sc.G == sc.g_from_gap(largest)
