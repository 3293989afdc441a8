"""CPU half of tests/test_optim_kernels_gpu.py: the float64 references written there agree with the
project's other two descriptions of each update rule (fused.fused_adam_ / fused.fused_momentum_ on
CPU tensors, DistributedFusedLamb._torch_update), and the tolerances used on the GPU are 8x the
measured distance of a plain fp32 evaluation from float64.

The agreement tests use hyper-parameters that fp32 holds exactly (beta2 = 1 - 2^-10, ...). The
references take the values the kernels get, i.e. rounded to fp32 (as Paddle's kernels, the HIP
kernels form 1 - beta2 from the fp32 beta2: 1 - float(0.999) is 1.00005e-3); the CPU paths form
1 - beta2 in double. With 0.999 the two differ by 5e-5 relative in v, which is a difference of
inputs, not of rules."""
import copy

import pytest
import torch

import test_optim_kernels_gpu as K

F32, F64 = torch.float32, torch.float64
SHAPES = [(1,), (257,), (1025,), (K.CHUNK + 1,), (37, 129), (0,)]
B1, B2 = 0.875, 1.0 - 2.0 ** -10
WDS, LR_RATIOS = (0.125, 0.0, 2.0 ** -7), (1.0, 0.5, 2.0, 0.125)


def _exact(hp):
    """the case with hyper-parameters that are fp32 numbers"""
    hp = dict(hp)
    for k, v in (("beta1", B1), ("beta2", B2), ("mu", B1), ("lr", 2.0 ** -6)):
        if k in hp:
            hp[k] = v
    if "eps" in hp:
        hp["eps"] = K.f32r(hp["eps"])
    hp["grad_scale"] = K.f32r(hp["grad_scale"])
    return hp


def _within(measured, tol, what):
    """The constant is 8x the measurement as recorded in the GPU file's header. Re-measured here it
    must still be that to within a factor of two either way: torch's fp32 sums depend on the
    host's vector width and thread count, so the figure moves a little between machines, while
    a case that changed without a new measurement, or a widened constant, moves it a lot."""
    print(f"{what}: measured {measured:.3e} x8 = {K.MARGIN * measured:.3e} bound {tol:.3e}")
    assert K.MARGIN / 2 * measured <= tol, what + ": bound tighter than the measurement supports"
    assert tol <= 2 * K.MARGIN * measured, what + ": bound wider than the measurement supports"


@pytest.mark.parametrize("rule,cases", [("adam", K.ADAM_CASES), ("momentum", K.MOM_CASES)])
def test_bounds_are_eight_times_the_fp32_distance(rule, cases):
    worst = K.measure(rule, cases)
    for k, (a, r) in worst.items():
        name = "vel" if (rule == "momentum" and k == "m") else k
        _within(a, K.TOL[rule][name][0], f"{rule} {name} atol")
        _within(r, K.TOL[rule][name][1], f"{rule} {name} rtol")


def test_lamb_bounds_are_eight_times_the_fp32_distance():
    worst = K.measure_lamb()
    for k, (a, r) in worst.items():
        if k != "norms":
            _within(a, K.TOL["lamb"][k][0], f"lamb {k} atol")
        _within(r, K.TOL["lamb"][k][1], f"lamb {k} rtol")
    _within(K.measure_lamb_sq(), K.TOL["lamb_sq"]["sum"][1], "lamb_sq rtol")


def _cpu_state(entries):
    ps = [e["p0"].clone() for e in entries]
    masters = [e["master0"].clone() if e["has_master"] else None for e in entries]
    return ps, [e["m0"].clone() for e in entries], [e["v0"].clone() for e in entries], masters


def _snap(ps, ms, vs, masters):
    c = lambda xs: [None if x is None else x.clone() for x in xs]   # noqa: E731
    return dict(p=c(ps), m=c(ms), v=c(vs), master=c(masters))


@pytest.mark.parametrize("combo", ["f32", "bf16_master", "mixed"])
@pytest.mark.parametrize("case", list(K.ADAM_CASES))
def test_ref_adam_matches_fused_cpu(case, combo):
    from paddle_hackathon_amd.ops import fused
    hp = _exact(K.ADAM_CASES[case])
    entries = K.make_entries(combo, 21, shapes=SHAPES, zero_state=hp["zero_state"], wds=WDS, lr_ratios=LR_RATIOS)
    ps, ms, vs, masters = _cpu_state(entries)
    snaps = []
    for k in range(K.NSTEPS):
        for i, e in enumerate(entries):   # per tensor, as optimizer.Adam calls the CPU path
            fused.fused_adam_([ps[i]], [e["grads"][k]], [ms[i]], [vs[i]], [masters[i]], hp["lr"], hp["beta1"],
                              hp["beta2"], hp["eps"], hp["step0"] + k, e["wd"], hp["decoupled"], [e["lr_ratio"]],
                              hp["grad_scale"])
        snaps.append(_snap(ps, ms, vs, masters))
    K.verify("adam", entries, hp, snaps, f"fused_adam_ cpu {case}/{combo}")


@pytest.mark.parametrize("combo", ["f32", "bf16_master", "mixed"])
@pytest.mark.parametrize("case", list(K.MOM_CASES))
def test_ref_momentum_matches_fused_cpu(case, combo):
    from paddle_hackathon_amd.ops import fused
    hp = _exact(K.MOM_CASES[case])
    entries = K.make_entries(combo, 22, shapes=SHAPES, wds=WDS, lr_ratios=LR_RATIOS)
    ps, vels, _, masters = _cpu_state(entries)
    snaps = []
    for k in range(K.NSTEPS):
        for i, e in enumerate(entries):
            fused.fused_momentum_([ps[i]], [e["grads"][k]], [vels[i]], [masters[i]], hp["lr"], hp["mu"],
                                  hp["nesterov"], e["wd"], [e["lr_ratio"]], hp["grad_scale"])
        snaps.append(_snap(ps, vels, [], masters))
    K.verify("momentum", entries, hp, snaps, f"fused_momentum_ cpu {case}/{combo}")


@pytest.mark.parametrize("clip", [0.0, 1.0, 1e4])
def test_ref_lamb_matches_torch_update(clip):
    import paddle_hackathon_amd as paddle
    from paddle_hackathon_amd.incubate import DistributedFusedLamb
    lay = K.layout("small")
    opt = DistributedFusedLamb(K.LAMB_LR, beta1=B1, beta2=B2, epsilon=K.LAMB_EPS,
                               parameters=paddle.nn.Linear(2, 2).parameters())
    F = dict(params=[None] * (lay["npar"] - 1), pid=lay["pid"].clone(), wd=lay["wd"].clone(),
             lr_ratio=lay["lr_ratio"].clone(), master=lay["w0"].clone(), m1=torch.zeros(lay["n"]),
             m2=torch.zeros(lay["n"]), b1p=1.0, b2p=1.0)
    ref = K.lamb_chain(lay, clip, 1.0, F64, b1=B1, b2=B2)
    tol = K.TOL["lamb"]
    for k in range(K.LAMB_STEPS):
        opt._torch_update(F, copy.deepcopy(lay["grads"][k]), 1, clip)
        K.check(F["master"], ref[k]["w"], tol["w"], f"_torch_update step {k} w")
        K.check(F["m1"], ref[k]["m1"], tol["m1"], f"_torch_update step {k} m1")
        K.check(F["m2"], ref[k]["m2"], tol["m2"], f"_torch_update step {k} m2")
    frozen = torch.isin(lay["pid"], torch.tensor(sorted(lay["frozen"])))
    assert torch.equal(F["master"][frozen], lay["w0"][frozen])
