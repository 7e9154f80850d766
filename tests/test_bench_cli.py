"""bench.py's command line: a plain run prints only the headline line and, with
``--dump-outputs``, writes what its last timed step returned; the output sample is seeded."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import bench

HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps",
                 "warmup", "n_gpus", "config"}
FULL_ONLY_KEYS = {"roofline", "rooflines_secondary", "end_to_end", "training_step", "cpu_baseline"}


def _fake_outputs(iters, batch, size, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(batch, 2, size, size), (batch, 2, size, size), (batch, 3, 3), (batch, 3),
              (batch, 1, size, size), (batch, 3, 3), (batch, 3)]
    return tuple([torch.randn(s, generator=g) for _ in range(iters)] for s in shapes)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    outs = _fake_outputs(3, 2, 16, seed=0)
    # 7 arrays share the budget: 200 elements each, so the flows (3·2·2·16² = 3072) and the mask
    # (1536) are sampled and the poses (54, 18) are written whole
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 7 * 4 * 200)
    bench.dump_outputs(outs, str(tmp_path / "a"))
    bench.dump_outputs(outs, str(tmp_path / "b"))
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in bench.OUTPUT_NAMES)
    total = 0
    for name, seq in zip(bench.OUTPUT_NAMES, outs):
        a = np.load(tmp_path / "a" / (name + ".npy"))
        whole = torch.stack(seq).numpy()
        total += a.nbytes
        assert a.dtype == np.float32
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy")))  # same positions
        if whole.size <= 200:
            assert np.array_equal(a, whole)
        else:
            idx = np.sort(np.random.default_rng(whole.size).integers(0, whole.size, size=200))
            assert np.array_equal(a, whole.reshape(-1)[idx])
    assert total <= 7 * 4 * 200


def _run_bench(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_headline_and_dumped_outputs(tmp_path, monkeypatch, capsys):
    """--batch 2 --iters 2 at 256²: the line holds the headline fields and none of --full's, and
    the dumped arrays are the decoder's forward on the bench's own inputs, bit for bit."""
    from scflow_amd import MODELS, synthetic
    out = tmp_path / "dump"
    res = _run_bench(monkeypatch, capsys, "--gpus", "1", "--steps", "2", "--warmup", "1",
                     "--batch", "2", "--iters", "2", "--dump-outputs", str(out))
    assert HEADLINE_KEYS <= set(res) and not FULL_ONLY_KEYS & set(res)
    assert res["steps"] == 2 and res["warmup"] == 1 and res["unit"] == "iters/s"
    assert res["higher_is_better"] is True and res["dtype"] == "f32" and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(2 * 2 / (res["ms_per_step"] * 1e-3), rel=5e-3)

    dec = MODELS.build(bench.decoder_cfg(2))
    synthetic.fill_module_(dec)
    dec = dec.cuda().eval()
    ref = dec(**bench.make_inputs(2, 256, seed=0, device="cuda"), invalid_flow_num=0.0)
    torch.cuda.synchronize()
    for name, seq in zip(bench.OUTPUT_NAMES, ref):
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float32
        assert np.array_equal(got, torch.stack(seq).float().cpu().numpy()), name
