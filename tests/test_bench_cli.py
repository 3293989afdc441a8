"""bench.py's command line: a plain run times only the headline model (the ResNet-50 half runs
under ``--full`` alone), ``--dump-outputs DIR`` writes the last step's loss and a fixed, seeded
sample of the parameters and their fp32 master weights as float32 ``.npy`` files."""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_cli_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _P:
    def __init__(self, t, name=None):
        self._t, self.name = t, name


class _Opt:
    def __init__(self, masters=None):
        self._m = masters

    def state_dict(self):
        return {"master_weights": self._m} if self._m else {}


def _parse(bench, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench._args()


def test_plain_run_is_lean_by_default(bench, monkeypatch):
    a = _parse(bench, monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = _parse(bench, monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"


def test_resnet_half_runs_only_under_full(bench, monkeypatch):
    def runs(*argv):
        return bench._runs_resnet_half(_parse(bench, monkeypatch, *argv))
    assert runs("--full") is True
    assert runs() is False
    assert runs("--no-resnet") is False
    assert runs("--full", "--no-resnet") is False
    assert runs("--full", "--model", "gpt3-13b") is False
    assert runs("--full", "--model", "bert-base") is False


def test_plain_gpt_run_never_enters_the_resnet_bench(bench, monkeypatch, capsys):
    """main() with the trainer and the device calls stubbed out: a plain run prints the result line
    without calling bench_resnet; a --full run calls it and reports config.resnet50_*"""
    import paddle_hackathon_amd as paddle
    import paddle_hackathon_amd.models.gpt_train as gt
    calls = []

    class Trainer:
        def __init__(self, *a, **k):
            self.cfg = types.SimpleNamespace(vocab_size=32)
            self.model = self.inner = types.SimpleNamespace(parameters=lambda: [])
            self.opt = _Opt()
            self.n_params = 0

        def data_rank(self):
            return 0

        def step(self, inp, lab):
            return torch.tensor(1.5)

    def fake_resnet(a, paddle, dist, world, rank, emit=True):
        calls.append(a.graph)
        return {"value": 1.0, "ms_per_step": 2.0,
                "config": {"samples_per_sec_per_gpu": 1.0, "global_batch": 256, "hip_graph": False}}

    real_randint, real_gen = torch.randint, torch.Generator
    monkeypatch.setattr(gt, "GPTTrainer", Trainer)
    monkeypatch.setattr(bench, "bench_resnet", fake_resnet)
    monkeypatch.setattr(bench, "_gpt_micro_batch", lambda *a: 2)
    monkeypatch.setattr(paddle, "set_device", lambda *a, **k: None)
    for name, fn in (("set_device", lambda *a, **k: None), ("current_device", lambda: 0),
                     ("synchronize", lambda *a, **k: None), ("empty_cache", lambda: None),
                     ("max_memory_allocated", lambda *a, **k: 0)):
        monkeypatch.setattr(torch.cuda, name, fn)
    monkeypatch.setattr(torch, "Generator", lambda device=None: real_gen())
    monkeypatch.setattr(torch, "randint", lambda lo, hi, size, device=None, generator=None:
                        real_randint(lo, hi, size, generator=generator))
    monkeypatch.delenv("WORLD_SIZE", raising=False)

    def run(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "2", "--warmup", "1", "--seq-len", "8", *argv])
        bench.main()
        return json.loads(capsys.readouterr().out.strip().splitlines()[-1])

    plain = run()
    assert calls == []
    assert plain["steps"] == 2 and plain["ms_per_step"] > 0 and plain["unit"] == "tokens/s"
    assert not [k for k in plain["config"] if k.startswith("resnet50_")]
    full = run("--full")
    assert calls == ["auto"]
    assert full["config"]["resnet50_samples_per_sec"] == 1.0
    assert {k for k in full if k != "config"} == {k for k in plain if k != "config"}
    run("--full", "--no-resnet")
    assert calls == ["auto"]


def test_dump_outputs_sample_is_fixed(bench, monkeypatch, tmp_path):
    n_big = 3 * bench._DUMP_PER_PARAM + 5
    big = torch.arange(n_big, dtype=torch.float32)
    params = [_P(big.to(torch.bfloat16).reshape(-1, 1), "w0"), _P(torch.arange(6, dtype=torch.float32).reshape(2, 3), "w1")]
    opt = _Opt({"w0": _P(big.clone())})
    loss = torch.tensor(2.5)
    for d in ("a", "b"):
        a = _parse(bench, monkeypatch, "--dump-outputs", str(tmp_path / d))
        bench._dump_outputs(a, 0, loss, params, opt)
    la, pa = np.load(tmp_path / "a" / "loss.npy"), np.load(tmp_path / "a" / "params_sample.npy")
    ma = np.load(tmp_path / "a" / "master_sample.npy")
    assert la.dtype == np.float32 and la.tolist() == [2.5]
    assert pa.dtype == np.float32 and pa.shape == (bench._DUMP_PER_PARAM + 6,)
    # small parameters whole, in order; large ones sampled at sorted positions of the flat tensor
    assert pa[-6:].tolist() == [0, 1, 2, 3, 4, 5]
    assert np.all(np.diff(pa[:-6]) >= 0) and pa[:-6].max() <= n_big
    # the master weights of the bf16 parameter, at the same positions, unrounded
    assert ma.dtype == np.float32 and ma.shape == (bench._DUMP_PER_PARAM,)
    assert np.array_equal(torch.from_numpy(ma).to(torch.bfloat16).float().numpy(), pa[:-6])
    assert np.any(ma != pa[:-6])
    for n in ("params_sample.npy", "master_sample.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
    # other ranks and runs without the option write nothing; no master weights, no master file
    bench._dump_outputs(_parse(bench, monkeypatch, "--dump-outputs", str(tmp_path / "c")), 1, loss, params, opt)
    bench._dump_outputs(_parse(bench, monkeypatch), 0, loss, params, opt)
    assert not (tmp_path / "c").exists()
    bench._dump_outputs(_parse(bench, monkeypatch, "--dump-outputs", str(tmp_path / "d")), 0, loss, params, _Opt())
    assert sorted(os.listdir(tmp_path / "d")) == ["loss.npy", "params_sample.npy"]


@pytest.mark.gpu
@pytest.mark.parametrize("argv", [["--model", "gpt-tiny", "--seq-len", "64"],
                                  ["--model", "bert-tiny", "--seq-len", "64", "--micro-batch", "2"],
                                  ["--model", "resnet50", "--micro-batch", "4"]],
                         ids=["gpt", "bert", "resnet"])
def test_dump_outputs_of_a_real_run(argv, tmp_path):
    """bench.py on the GPU at the smallest sizes, once per model family: the files are there, finite,
    float32, within the size limit, and loss.npy is the loss of the result line where that has one"""
    env = {k: v for k, v in os.environ.items() if k != "WORLD_SIZE"}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)] + argv, cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    assert not [k for k in res["config"] if k.startswith("resnet50_")]
    files = {n: np.load(tmp_path / n) for n in sorted(os.listdir(tmp_path))}
    assert sorted(files) == ["loss.npy", "master_sample.npy", "params_sample.npy"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in files.values())
    assert 0 < sum(v.nbytes for v in files.values()) <= 64 * 2 ** 20
    assert files["loss.npy"].shape == (1,)
    if "final_loss" in res["config"]:   # rounded to 4 places in the result line
        assert abs(float(files["loss.npy"][0]) - res["config"]["final_loss"]) <= 5.1e-5
    assert 0 < files["master_sample.npy"].size <= files["params_sample.npy"].size
