"""Write a small synthetic set of channel impulse responses for ``-channel dataset`` (neural_rx_amd/cir.py).

    python tools/make_cir_dataset.py --out cir_toy.npz [--examples 256] [--paths 32] [--seed 1]
    python tools/make_cir_dataset.py --out flat.npz --flat

THIS IS A TOY.  It is a few lines of single-bounce geometry so that the documented command lines run without external
data; it is no ray tracer, no 3GPP model and no measured site, and curves on it say nothing about any real deployment.

Geometry (numpy, seeded): a base station at the origin with ``--antennas`` elements on a half-wavelength uniform
linear array along x; ``--paths - 1`` fixed point scatterers in a 200 m x 200 m area in front of it; two users, each
walking a straight line (its "trajectory") at 3 and 30 m/s.  Example ``e`` is user ``e % 2`` at step ``e // 2`` of its
line, so ``-cir_select trajectory`` keeps evaluation user u on trajectory u.  Every example has a line-of-sight path
and one path over every scatterer:

    delay        (d_user_scatterer + d_scatterer_bs) / c, minus the example's shortest delay (the first path is at 0)
    power        falls with the delay: free-space loss over the whole path length, 1 / (d1 + d2)^2 (a specular bounce),
                 and a log-normal reflection loss of 6 +- 3 dB per scatterer
    array        exp(-j pi a cos(phi)), phi the angle of arrival of the path at the array, a the element
    Doppler      exp(j 2 pi f_D t T_sym) over the 14 symbols, f_D = (v / lambda) cos(angle of the user's velocity to
                 its departure direction), T_sym = 1.07 / subcarrier spacing

``--flat`` writes two one-path unit channels instead (no delay, two orthogonal beams over the array; cir.one_path):
with ``-cir_select trajectory`` the channel on which a receiver with perfect channel knowledge makes no error without
noise.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C0 = 299792458.0


def make(examples=256, antennas=4, paths=32, seed=1, carrier_hz=3.5e9, subcarrier_spacing=30e3):
    """(a complex64 [E, A, L, 14], tau float32 [E, L])"""
    rng = np.random.default_rng(seed)
    lam = C0 / carrier_hz
    tsym = 1.07 / subcarrier_spacing
    scat = np.stack([rng.uniform(-100.0, 100.0, paths - 1), rng.uniform(20.0, 220.0, paths - 1)], -1)     # [L-1, 2]
    loss = 10.0 ** (-rng.normal(6.0, 3.0, paths - 1) / 20.0)                                              # amplitude
    refl = np.exp(2j * np.pi * rng.uniform(0, 1, paths - 1))
    start = np.array([[-60.0, 80.0], [50.0, 150.0]])
    heading = np.array([[1.0, 0.2], [-0.6, -0.8]])
    heading /= np.linalg.norm(heading, axis=1, keepdims=True)
    speed = np.array([3.0, 30.0])
    steps = (examples + 1) // 2
    a = np.zeros((examples, antennas, paths, 14), np.complex128)
    tau = np.zeros((examples, paths))
    t = np.arange(14) * tsym
    for e in range(examples):
        u, k = e % 2, e // 2
        pos = start[u] + heading[u] * (40.0 * k / max(steps - 1, 1))          # 40 m of each line
        via = np.concatenate([np.zeros((1, 2)), scat])                         # the point the path reaches the array from
        d2 = np.linalg.norm(via, axis=1)                                       # scatterer -> array (0 for the LOS row)
        dep = np.concatenate([-pos[None], scat - pos[None]])                   # user -> first point of the path
        d1 = np.linalg.norm(dep, axis=1)
        dist = d1 + d2
        amp = np.concatenate([[1.0], loss]) * lam / (4 * np.pi * dist)
        arr = np.concatenate([pos[None], scat])                                # where the array sees the path come from
        cosphi = arr[:, 0] / np.linalg.norm(arr, axis=1)
        fd = speed[u] / lam * (dep @ heading[u]) / d1
        g = amp * np.concatenate([[1.0], refl]) * np.exp(-2j * np.pi * dist / lam)
        steer = np.exp(-1j * np.pi * np.arange(antennas)[:, None] * cosphi[None, :])
        a[e] = (g[None, :] * steer)[:, :, None] * np.exp(2j * np.pi * fd[:, None] * t[None, :])[None]
        tau[e] = (dist - dist.min()) / C0
        order = np.argsort(tau[e], kind="stable")
        a[e], tau[e] = a[e][:, order], tau[e][order]
    a /= np.sqrt(np.mean(np.sum(np.abs(a) ** 2, axis=2)))                      # unit mean energy per antenna and symbol
    return a.astype(np.complex64), tau.astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description="a TOY channel-impulse-response dataset for -channel dataset")
    ap.add_argument("--out", required=True)
    ap.add_argument("--examples", type=int, default=256)
    ap.add_argument("--antennas", type=int, default=4)
    ap.add_argument("--paths", type=int, default=32, help="one line-of-sight path and paths - 1 scatterers (2..1024)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--flat", action="store_true", help="the one-path unit channel instead")
    args = ap.parse_args()
    from neural_rx_amd.cir import CIRDataset, one_path
    if args.flat:
        ds = one_path(args.antennas, 2)
    else:
        if not 2 <= args.paths <= 1024 or args.examples < 2:
            ap.error("need 2..1024 paths and at least 2 examples (one per trajectory)")
        ds = CIRDataset(*make(args.examples, args.antennas, args.paths, args.seed))
    ds.save(args.out)
    print(f"{args.out}: a TOY dataset, {ds.num_examples} examples x {ds.num_rx_ant} antennas x {ds.num_paths} paths x "
          f"{ds.num_time_steps} time steps; max delay {float(ds.tau.max()) * 1e9:.0f} ns")


if __name__ == "__main__":
    main()
