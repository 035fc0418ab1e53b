"""``python -m neural_rx_amd.evaluate -channel dataset`` on a dataset of tools/make_cir_dataset.py (needs an MI355X)."""
import importlib.util
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["perf_csi_lmmse", "lmmse_lmmse"]


def _tool():
    spec = importlib.util.spec_from_file_location("make_cir_dataset", os.path.join(ROOT, "tools", "make_cir_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _argv(path, ebno, *more):
    return ["-config_name", "nrx_rt", "-num_tx_eval", "2", "-num_prbs", "4", "-ebno_db", str(ebno), "-batch_size", "8",
            "-max_mc_iter", "2", "-num_cov_slots", "32", "-channel", "dataset", "-cir_file", path, "-baselines"] + NAMES \
        + list(more)


def test_evaluate_on_the_toy_dataset(tmp_path):
    from neural_rx_amd import evaluate
    from neural_rx_amd.cir import CIRDataset
    path = str(tmp_path / "toy.npz")
    a, tau = _tool().make(examples=64, antennas=4, paths=24, seed=3)
    CIRDataset(a, tau).save(path)
    back = CIRDataset.load(path)
    np.testing.assert_array_equal(back.a, a)
    np.testing.assert_array_equal(back.tau, tau)
    with np.load(path) as z:
        assert sorted(z.files) == ["a", "tau"]
    d = evaluate.main(_argv(path, 6.0, "-cir_select", "trajectory"))
    assert d["channel"] == "dataset" and d["chest"] == "lmmse3" and d["mc_iters"] == [2]
    assert d["cir"]["num_examples"] == 64 and d["cir"]["num_paths"] == 24 and d["cir"]["select"] == "trajectory"
    assert d["cir"]["f_offset"] == -24.0 and d["cir"]["normalize"] is True
    assert list(d["baselines"]) == NAMES
    bers = [d["ber"][0]] + [d["baselines"][n]["ber"][0] for n in NAMES]
    print("BER nrx / perf_csi_lmmse / lmmse_lmmse:", bers)
    assert all(math.isfinite(b) and 0.0 <= b <= 0.5 for b in bers)
    for n in NAMES:
        assert d["baselines"][n]["counts"][0][1] == d["counts"][0][1]      # paired: the same bits
    two_d = evaluate.main(_argv(path, 6.0, "-chest_2d", "-cir_no_norm", "-cir_f_zero"))
    assert two_d["chest"] == "lmmse" and two_d["cir"]["f_offset"] == 0.0 and two_d["cir"]["normalize"] is False
    assert math.isfinite(two_d["baselines"]["lmmse_lmmse"]["ber"][0])


def test_perfect_csi_makes_no_error_on_a_flat_channel_at_40_db(tmp_path):
    from neural_rx_amd import evaluate
    from neural_rx_amd.cir import one_path
    path = str(tmp_path / "flat.npz")
    one_path(4, 2).save(path)
    # two examples on orthogonal beams, user u on example u: a one-path channel has rank one per user
    d = evaluate.main(_argv(path, 40.0, "-cir_select", "trajectory"))
    c = d["baselines"]["perf_csi_lmmse"]["counts"]
    print("perf_csi_lmmse counts at 40 dB:", c, "nrx BER", d["ber"][0])
    assert c[0][1] > 0 and c[0][0] == 0
    assert all(math.isfinite(d["baselines"][n]["ber"][0]) for n in NAMES) and math.isfinite(d["ber"][0])


def test_the_dataset_excludes_the_correlated_scenarios(tmp_path):
    from neural_rx_amd import evaluate
    from neural_rx_amd.cir import one_path
    path = str(tmp_path / "flat.npz")
    one_path(4, 2).save(path)
    for argv in (_argv(path, 6.0, "-rx_corr", "0.5"),
                 ["-channel", "double_tdl_low", "-cir_file", path], ["-channel", "dataset"]):
        with pytest.raises(SystemExit):
            evaluate.main(argv)
