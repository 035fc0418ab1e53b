"""The host side of the training loop (neural_rx_amd/train.py, config.parse_schedule): the schedule parser, the
active-user law, the slot accounting and the (seed, step)-keyed draws.  No GPU."""
import glob
import os

import numpy as np
import pytest

from neural_rx_amd import train
from neural_rx_amd.config import ScheduleStage, parse_schedule

CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config")
CFGS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CFG_DIR, "*.cfg")))


def test_the_five_cfgs_are_there():
    assert CFGS == ["nrx_large.cfg", "nrx_large_64qam.cfg", "nrx_large_var_mcs_64qam_masking.cfg", "nrx_rt.cfg",
                    "nrx_rt_var_mcs.cfg"]


def test_parse_schedule_nrx_rt():
    s = parse_schedule(os.path.join(CFG_DIR, "nrx_rt.cfg"))
    assert (s.min_num_tx, s.max_num_tx) == (1, 2)
    assert s.stages == (
        ScheduleStage(num_iter=1000000, learning_rate=0.001, batch_size=128, min_training_snr_db=(0.0, 0.0),
                      max_training_snr_db=(10.0, 15.0), double_readout=True, apply_multiloss=False,
                      weighting_double_readout=0.02),
        ScheduleStage(num_iter=9000000, learning_rate=0.001, batch_size=128, min_training_snr_db=(1.0, 2.0),
                      max_training_snr_db=(7.0, 12.0), double_readout=True, apply_multiloss=False,
                      weighting_double_readout=0.01))
    assert s.total_steps == 10 ** 7 and [st.w_chest for st in s.stages] == [0.02, 0.01]
    assert all(type(st.num_iter) is int and type(st.batch_size) is int for st in s.stages)
    t = s.scaled(1e-4)
    assert [st.num_iter for st in t.stages] == [100, 900] and t.stages[1].learning_rate == 0.001
    assert t.stage_of(0)[0] == 0 and t.stage_of(99)[0] == 0 and t.stage_of(100)[0] == 1 and t.stage_of(999)[0] == 1
    with pytest.raises(IndexError):
        t.stage_of(1000)
    assert [st.num_iter for st in s.scaled(1e-9).stages] == [1, 1]


@pytest.mark.parametrize("name", CFGS)
def test_parse_schedule_every_cfg(name):
    s = parse_schedule(os.path.join(CFG_DIR, name))
    assert (s.min_num_tx, s.max_num_tx) == (1, 2)
    assert len(s.stages) == (3 if name == "nrx_rt_var_mcs.cfg" else 2)
    for st in s.stages:
        assert st.batch_size == 128 and st.num_iter >= 100000 and st.learning_rate in (0.001, 0.0005)
        assert len(st.min_training_snr_db) == len(st.max_training_snr_db) == 2
        assert all(a < b for a, b in zip(st.min_training_snr_db, st.max_training_snr_db))
        assert st.double_readout and st.weighting_double_readout in (0.02, 0.01)
        assert st.apply_multiloss == name.startswith("nrx_large")
    if name == "nrx_rt_var_mcs.cfg":
        assert [st.num_iter for st in s.stages] == [100000, 2000000, 7000000]
        assert [st.learning_rate for st in s.stages] == [0.0005, 0.001, 0.0005]
        assert s.stages[2].min_training_snr_db == (-2.0, 0.0) and s.stages[2].max_training_snr_db == (3.0, 5.0)


def _edited(tmp_path, old, new):
    text = open(os.path.join(CFG_DIR, "nrx_rt.cfg")).read()
    assert old in text
    p = tmp_path / "edited.cfg"
    p.write_text(text.replace(old, new))
    return str(p)


def test_parse_schedule_refusals(tmp_path):
    with pytest.raises(ValueError, match="train_tx"):
        parse_schedule(_edited(tmp_path, '"train_tx": [False, False]', '"train_tx": [False, True]'))
    # literal_eval, never eval: an expression is no literal
    with pytest.raises(ValueError):
        parse_schedule(_edited(tmp_path, '"num_iter": [1e6, 9e6]', '"num_iter": [__import__("os").getpid(), 9e6]'))
    with pytest.raises(ValueError, match="one entry per stage"):
        parse_schedule(_edited(tmp_path, '"batch_size": [128, 128]', '"batch_size": [128]'))
    with pytest.raises(ValueError, match="SNR range"):
        parse_schedule(_edited(tmp_path, "[[0., 0.],[1., 2.]]", "[[0.],[1., 2.]]"))
    with pytest.raises(ValueError, match="lacks"):
        parse_schedule(_edited(tmp_path, '"learning_rate": [0.001, 0.001],', ""))


# ---------------------------------------------------------------- the active-user law
N_DRAWS = 100000


@pytest.fixture(scope="module")
def uniforms():
    """the uniform of the active-user draw of steps 0..N_DRAWS-1 at seed 7, as the loop takes it"""
    return np.array([train._step_rng(train._DRAW_NUM_TX, 7, k).random() for k in range(N_DRAWS)])


def law_probabilities(a, b):
    """P(n) for n = floor(a + sqrt(u) w), w = b + 1 - a: n <= j iff u < ((j + 1 - a) / w)^2"""
    w = b + 1 - a
    cdf = [((j + 1 - a) / w) ** 2 for j in range(a - 1, b + 1)]
    return {n: cdf[n - a + 1] - cdf[n - a] for n in range(a, b + 1)}


def test_law_probabilities_of_one_to_two():
    assert law_probabilities(1, 2) == {1: 0.25, 2: 0.75}


@pytest.mark.parametrize("a,b", [(1, 2), (1, 4)])
def test_active_user_law(uniforms, a, b):
    n = train.num_tx_law(uniforms, a, b)
    assert n.min() >= a and n.max() <= b
    for v, p in law_probabilities(a, b).items():
        count, sigma = int((n == v).sum()), np.sqrt(N_DRAWS * p * (1 - p))
        print(f"{a}..{b}: n = {v}  count {count}  expected {N_DRAWS * p:.0f}  sigma {sigma:.1f}")
        assert abs(count - N_DRAWS * p) <= 4 * sigma
    # the loop's draw is this law on this uniform
    for k in (0, 1, 17, N_DRAWS - 1):
        assert train.sample_num_tx(7, k, a, b) == n[k]
    # the ends of the unit interval
    assert train.num_tx_law(0.0, a, b) == a and train.num_tx_law(np.nextafter(1.0, 0.0), a, b) == b


# ---------------------------------------------------------------- slot accounting and the resume property
SPLITS = [(7, 2, 2), (8, 3, 3), (5, 1, 5)]


@pytest.mark.parametrize("Bg,world,micro", SPLITS)
def test_micro_batches_partition_the_step(Bg, world, micro):
    for k in (0, 3, 10 ** 6):
        pieces = [r for rank in range(world) for r in train.micro_ranges(k, Bg, world, rank, micro)]
        assert all(0 < hi - lo <= micro for lo, hi in pieces)
        assert pieces[0][0] == k * Bg and pieces[-1][1] == (k + 1) * Bg
        assert all(p[1] == q[0] for p, q in zip(pieces, pieces[1:]))        # contiguous, in order, no overlap
    if (Bg, world, micro) == (7, 2, 2):
        assert train.micro_ranges(1, 7, 2, 0, 2) == [(7, 9), (9, 11)] and train.micro_ranges(1, 7, 2, 1, 2) == [(11, 13), (13, 14)]
    assert train.micro_ranges(2, Bg, 1, 0, 0) == [(2 * Bg, 3 * Bg)]         # 0: the whole shard in one piece


@pytest.mark.parametrize("Bg,world,micro", SPLITS)
def test_ebno_is_one_array_whichever_rank_draws_it(Bg, world, micro):
    k = 5
    whole = train.step_ebno_db(11, k, Bg, 1.0, 7.0)
    assert whole.shape == (Bg,) and whole.dtype == np.float64 and (whole >= 1.0).all() and (whole <= 7.0).all()
    assert len(set(whole.tolist())) == Bg
    seen = []
    for rank in range(world):
        mine = train.step_ebno_db(11, k, Bg, 1.0, 7.0)       # every rank draws the step's array for itself
        for lo, hi in train.micro_ranges(k, Bg, world, rank, micro):
            seen.append(mine[lo - k * Bg:hi - k * Bg])
    assert np.concatenate(seen).tobytes() == whole.tobytes()
    one = train.step_ebno_db(11, k, Bg, 1.0, 7.0, per_slot=False)
    assert one.shape == (Bg,) and len(set(one.tolist())) == 1


def test_step_draws_do_not_depend_on_earlier_steps():
    """the resume property on the host: step k drawn first is step k drawn after steps 0..k-1"""
    straight = [(train.sample_num_tx(3, k, 1, 2), train.step_ebno_db(3, k, 6, 0.0, 10.0).tobytes()) for k in range(8)]
    for k in (7, 4, 0):
        assert (train.sample_num_tx(3, k, 1, 2), train.step_ebno_db(3, k, 6, 0.0, 10.0).tobytes()) == straight[k]
    assert len({e for _, e in straight}) == 8                          # ... and the steps differ
    assert train.step_ebno_db(4, 0, 6, 0.0, 10.0).tobytes() != straight[0][1]      # ... as do the seeds


def test_ebno_db_to_no_is_the_generators():
    from neural_rx_amd.generator import ebno_to_no
    e = np.array([-2.0, 0.0, 3.5, 12.0])
    assert np.allclose(train.ebno_db_to_no(e, 2), [ebno_to_no(float(x), 2) for x in e], rtol=1e-15, atol=0)


def test_new_command_line_refusals(capsys):
    for argv, word in ((["-num_gpus", "17"], "-num_gpus"), (["-num_gpus", "0"], "-num_gpus"),
                       (["-micro_batch", "-1"], "-micro_batch"), (["-schedule_scale", "0"], "-schedule_scale"),
                       (["-save_every", "5"], "needs -out")):
        with pytest.raises(SystemExit):
            train.main(argv)
        assert word in capsys.readouterr().err, argv
