"""CPU checks of the host-side rules every route shares (no GPU: recorders stand in for the plans):

* the scalar threshold rule (watroo/wavelets.py:129-143) - wavelets._tau_row against a transcription of the reference
  written out here;
* where utils._denoise_pipelined puts the threshold step, which thresholds and weights it hands to
  wt_denoise_sum_host, and when it refuses;
* the per-scale sigma_bilateral list (watroo/wavelets.py:421-424, utils.py:140-146), one rule under four names;
* the per-scale sequence of the bilateral transform (watroo/wavelets.py:433-442): the plan calls of the four
  routes that run it scale by scale, against call lists written out here."""
import itertools

import numpy as np
import pytest

from oracle import atrous_numpy as O
from wavelets_amd import _lib as L
from wavelets_amd import utils as WU
from wavelets_amd import wavelets as WV

SIGMAS = [0, 5, 3, -2, 1.5, np.float32(2)]
NOISES = [0, 0.7, -0.3, np.float32(1.25), np.float64(3)]
FAMILIES = [WV.Triangle, WV.B3spline]


def reference_tau(sigma, noise, sigma_e_scale, soft):
    """watroo/wavelets.py:129-143 for a scalar noise level, as the threshold t the kernels apply - erf(|w| / t)
    (soft) or |w| > t (hard) - with 0.0 standing for a significance of one everywhere."""
    if sigma != 0:                                               # :130
        if noise == 0:                                           # :133-135: np.ones_like
            return 0.0
        t = sigma * noise * sigma_e_scale                        # the divisor of :137, the bound of :141
        if soft:
            return float(abs(t))                                 # :137-138: erf(|w / t|) = erf(|w| / |t|)
        return float(t) if t > 0 else 0.0                        # :141: |w| > t holds everywhere for t < 0
    return 0.0                                                   # :142-143: np.ones_like


def same_floats(got, want):
    return [type(v) for v in got] == [float] * len(want) and list(got) == list(want)


@pytest.mark.parametrize("soft", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_tau_row_is_the_reference_threshold_rule(family, soft):
    sigma_e = family(2).sigma_e()
    for noise in NOISES:
        entries = [(scl, sig, 1) for scl in range(9) for sig in SIGMAS]          # every sigma at every scale 0..8
        want = [reference_tau(sig, noise, sigma_e[scl], soft) for scl, sig, _ in entries]
        got = WV._tau_row(entries, noise, sigma_e, soft)
        assert same_floats(got, want), (noise, got, want)
    assert any(t < 0 for t in (s * n for s in SIGMAS for n in NOISES))           # premise: negative products occur


def sigma_patterns(level, rng):
    """sigma lists of `level` entries: no threshold at all, one non-zero entry in front / at the end, random draws"""
    out = [[0] * level]
    for sig in SIGMAS[1:]:
        out.append([sig] + [0] * (level - 1))
        out.append([0] * (level - 1) + [sig])
    for _ in range(8):
        n = int(rng.integers(1, level + 1))
        out.append([SIGMAS[i] for i in rng.integers(0, len(SIGMAS), n)] + [0] * (level - n))
    return out


class PipelinePlan:
    """what utils._denoise_pipelined asks of a plan; anything else it touches is an AttributeError"""
    custom = False
    shape = (2048, 2048)

    def __init__(self, family):
        self.family = family
        self.calls = []

    def fused_ok(self, level):
        return True

    def denoise_sum_host(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return "piped"


def test_pipelined_denoise_places_the_threshold_step_and_refuses_as_transcribed():
    img = np.zeros(PipelinePlan.shape, np.float32)                # 1 << 22 pixels: the size guard's minimum
    rng = np.random.default_rng(11)
    kinds = {"piped": 0, "no non-zero sigma": 0, "single pass": 0, "every pass before the step": 0}
    cases = itertools.cycle(itertools.product(NOISES, (True, False)))
    for family in FAMILIES:
        sf = family(2)
        sigma_e = sf.sigma_e()
        for level in range(2, 9):
            sched = L.schedule(family._family, level, True)
            assert sum(n for _, n, _ in sched) == level
            for sigma in sigma_patterns(level, rng):
                noise, soft = next(cases)
                # the transcription: the threshold step goes behind the first k passes, the fewest (one at least)
                # that produce every plane with a non-zero sigma (Coefficients.denoise, :145-149, visits
                # len(sigma) planes; a zero sigma leaves its plane alone, :142-143)
                n_den = max([s + 1 for s, sig in enumerate(sigma) if sig != 0], default=0)
                k, covered = 0, 0
                while k < len(sched) and (covered < n_den or k == 0):
                    covered += sched[k][1]
                    k += 1
                if n_den == 0:
                    kind = "no non-zero sigma"
                elif len(sched) == 1:
                    kind = "single pass"
                elif k == len(sched):
                    kind = "every pass before the step"
                else:
                    kind = "piped"
                kinds[kind] += 1
                plan = PipelinePlan(family._family)
                given = list(sigma)
                got = WU._denoise_pipelined(plan, img, level, sf, sigma, noise, None, soft, False)
                assert sigma == given
                if kind != "piped":
                    assert got is None and plan.calls == [], (kind, level, sigma)
                    continue
                assert got == "piped" and len(plan.calls) == 1
                (a_img, a_level, a_k, a_taus, a_wgts, a_soft), kwargs = plan.calls[0]
                want = [reference_tau(sigma[s], noise, sigma_e[s], soft) for s in range(covered)]
                assert a_img is img and (a_level, a_k, a_soft) == (level, k, soft) and kwargs == {"out": None}
                assert same_floats(a_taus, want), (level, sigma, noise, soft, a_taus, want)
                assert same_floats(a_wgts, [1.0] * covered)
    assert all(n > 0 for n in kinds.values()), kinds              # premise: the pipeline and every refusal occur


def test_sigma_bilateral_list_is_one_rule_under_every_name():
    for given, n, want in ((2, 4, [2, 2, 2, 2, 2]),               # a scalar: repeated
                           ([1, 2], 4, [1, 2, 1, 1, 1]),          # a short list: padded with 1
                           ([1, 2, 3, 4, 5], 4, [1, 2, 3, 4, 5]),   # an exact list
                           ([1, 2, 3, 4, 5, 6, 7], 4, [1, 2, 3, 4, 5, 6, 7])):   # a long list: kept whole
        kept = list(given) if type(given) is list else given
        for rule in (WU._wow_sigma_bilateral, WV._sigma_bilateral_list, O._sigma_bilateral_list,
                     lambda b, lvl: WV.AtrousTransform(WV.B3spline, bilateral=b)._sigma_bilateral(lvl)):
            got = rule(given, n)
            assert got == want and type(got) is list and got is not given
            assert given == kept                                   # the caller's list is not touched
    assert WU._wow_sigma_bilateral(None, 4) is None


# ---- the per-scale bilateral sequence -------------------------------------------------------------------
IN, TMP = WV.PLANE_INPUT, WV._TMP_PLANE
S0 = WV.PLANE_SCRATCH(0)
REV = L.FLAG_TAPS_REVERSED
SEQUENCE_CALLS = ("set_border", "local_variance", "local_variance3d", "bilateral_conv", "bilateral3d_conv", "binary",
                  "decompose", "decompose3d", "decompose_bilateral", "copy")


def recording_plans(monkeypatch):
    """acquire_plan / acquire_plan64 hand out recorders; returns the list their calls go to, as
    (plan number, method, *arguments)"""
    calls = []

    class Recorder:
        def __init__(self, H, W, level):
            self.H, self.W, self.max_level, self.shape = H, W, level, (H, W)
            self.number = len({c[0] for c in calls if c[1] == "acquired"})
            calls.append((self.number, "acquired"))

        def __getattr__(self, name):
            if name.startswith("_"):
                raise AttributeError(name)
            return lambda *args: calls.append((self.number, name) + args)

    class Recorder32(Recorder):
        pass

    class Recorder64(Recorder):
        pass

    monkeypatch.setattr(WV, "Plan", Recorder32)
    monkeypatch.setattr(WV, "Plan64", Recorder64)
    monkeypatch.setattr(WV, "default_context", lambda: "ctx")
    monkeypatch.setattr(WV, "acquire_plan", lambda ctx, H, W, fam, level: Recorder32(H, W, level))
    monkeypatch.setattr(WV, "acquire_plan64", lambda ctx, H, W, taps, level: Recorder64(H, W, level))
    monkeypatch.setattr(WV, "release_plan", lambda plan: None)
    return calls


# Expected calls over two scales with bilateral=[1, 2] and bilateral_scaling=True, per scale s (:433-442):
#   variance = sdev_loc(c_s, s) * sigma_bilateral[s]**2 (:434: factors 1.0, 4.0), times s + 1 (:435-436: 1.0, 2.0)
#   c_{s+1} = the range-weighted convolution of c_s (:439-440);  w_s = c_s - c_{s+1} (:442)
# The smooth planes go input -> scratch 0 -> plane 2.  Border codes of a plan: 0 symmetric (np.pad of :77), 2 the
# 'mirror' border of convolution()'s 1-D branch (:65-69); 1 and 3 are the same two inside every polyphase sub-array
# (the recursive algorithm filters each on its own, :354-390, and the code puts border 0 back when it is done).  A
# signal's plan holds the taps reversed, which the range-weighted kernel is told (REV).  The recursive algorithm
# pads by 2 * 2**(level - 1) = 4 samples on every side: the cube of 6 slices has 14 there.
STANDARD_1D = [
    ("set_border", 2), ("local_variance", IN, TMP, 0, 1.0, 1.0),
    ("set_border", 0), ("bilateral_conv", IN, TMP, S0, 0, REV),
    ("binary", "sub", IN, S0, 0),
    ("set_border", 2), ("local_variance", S0, TMP, 1, 4.0, 2.0),
    ("set_border", 0), ("bilateral_conv", S0, TMP, 2, 1, REV),
    ("binary", "sub", S0, 2, 1)]
STANDARD_3D = [                                                   # (cubes: the 3-D operators, no border call)
    ("local_variance3d", IN, TMP, 0, 6, 1.0, 1.0), ("bilateral3d_conv", IN, TMP, S0, 0, 6),
    ("binary", "sub", IN, S0, 0),
    ("local_variance3d", S0, TMP, 1, 6, 4.0, 2.0), ("bilateral3d_conv", S0, TMP, 2, 1, 6),
    ("binary", "sub", S0, 2, 1)]
RECURSIVE_1D = [
    ("set_border", 3), ("local_variance", IN, TMP, 0, 1.0, 1.0),
    ("set_border", 1), ("bilateral_conv", IN, TMP, S0, 0, REV),
    ("binary", "sub", IN, S0, 0),
    ("set_border", 3), ("local_variance", S0, TMP, 1, 4.0, 2.0),
    ("set_border", 1), ("bilateral_conv", S0, TMP, 2, 1, REV),
    ("binary", "sub", S0, 2, 1),
    ("set_border", 0)]
RECURSIVE_2D = [
    ("set_border", 1), ("local_variance", IN, TMP, 0, 1.0, 1.0),
    ("set_border", 1), ("bilateral_conv", IN, TMP, S0, 0, 0),
    ("binary", "sub", IN, S0, 0),
    ("set_border", 1), ("local_variance", S0, TMP, 1, 4.0, 2.0),
    ("set_border", 1), ("bilateral_conv", S0, TMP, 2, 1, 0),
    ("binary", "sub", S0, 2, 1),
    ("set_border", 0)]
RECURSIVE_3D = [                                                  # (one border call per scale, ahead of the variance)
    ("set_border", 1), ("local_variance3d", IN, TMP, 0, 14, 1.0, 1.0), ("bilateral3d_conv", IN, TMP, S0, 0, 14),
    ("binary", "sub", IN, S0, 0),
    ("set_border", 1), ("local_variance3d", S0, TMP, 1, 14, 4.0, 2.0), ("bilateral3d_conv", S0, TMP, 2, 1, 14),
    ("binary", "sub", S0, 2, 1),
    ("set_border", 0)]

BILATERAL_CASES = [
    ("float32 1-D", np.float32, (40,), False, STANDARD_1D),
    ("float32 3-D", np.float32, (6, 10, 12), False, STANDARD_3D),
    ("float64 1-D", np.float64, (40,), False, STANDARD_1D),
    ("float64 3-D", np.float64, (6, 10, 12), False, STANDARD_3D),
    ("float32 recursive 1-D", np.float32, (40,), True, RECURSIVE_1D),
    ("float32 recursive 2-D", np.float32, (20, 24), True, RECURSIVE_2D),
    ("float32 recursive 3-D", np.float32, (6, 10, 12), True, RECURSIVE_3D),
    ("float64 recursive 1-D", np.float64, (40,), True, RECURSIVE_1D),
    ("float64 recursive 2-D", np.float64, (20, 24), True, RECURSIVE_2D),
    ("float64 recursive 3-D", np.float64, (6, 10, 12), True, RECURSIVE_3D),
]


@pytest.mark.parametrize("name,dtype,shape,recursive,want", BILATERAL_CASES, ids=[c[0] for c in BILATERAL_CASES])
def test_bilateral_transform_issues_the_per_scale_sequence(monkeypatch, name, dtype, shape, recursive, want):
    calls = recording_plans(monkeypatch)
    transform = WV.AtrousTransform(WV.B3spline, bilateral=[1, 2], bilateral_scaling=True)
    coefficients = transform(np.ones(shape, dtype), 2, recursive=recursive)
    assert len(coefficients) == 3 and coefficients._dtype == dtype
    # the plan that runs the sequence is the first one acquired (the recursive algorithm's padded one)
    got = [c[1:] for c in calls if c[0] == 0 and c[1] in SEQUENCE_CALLS]
    assert got == want, got
    assert [[type(v) for v in c] for c in got] == [[type(v) for v in c] for c in want]     # (the factors: Python floats)
