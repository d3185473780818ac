"""The float64 scan behind tests/_marginal_observe_ref.py's SIGMA and CUT (CPU only): per front-end case, K and candidate sigma,
the fp32 floors of grad_x / grad_c / grad_noise_std and by how much each damaged reference misses the bar of 22 floors.

    python scratch/marginal_observe_sigma_scan.py [sigma ...]
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tests import _marginal_observe_ref as O  # noqa: E402
from tests._pushforward_ref import normalised_error  # noqa: E402

FACTOR = 22.0


def damaged(r64):
    K = r64.wn.shape[1]
    return {"uniform": O.weighted(r64, torch.full_like(r64.wn, 1.0 / K)), "rolled": O.weighted(r64, r64.wn.roll(1, 0)),
            "no-z": O.weighted(r64, r64.wn, None), "p-for-z": O.weighted(r64, r64.wn, "p")}


def main():
    sigmas = [float(s) for s in sys.argv[1:]] or [0.1, 0.2, 0.3, 0.5, 0.8]
    for ck in O.CASES:
        for s in sigmas:
            r = O.references(ck, "cpu", s)
            r32, r64 = r[torch.float32], r[torch.float64]
            fl = O.floors(r32, r64)
            dm = damaged(r64)
            line = [f"{O.case_id(ck)} sigma {s}: min wn {float(r64.wn.min()):.2e} ess {float(r64.ess.min()):.2f}"]
            for i, what in enumerate(("gx", "gc", "gs")):
                if what not in fl:
                    continue
                ref = getattr(r64, what)
                names = ("uniform", "rolled") if what != "gs" else ("uniform", "rolled", "no-z", "p-for-z")
                miss = {n: normalised_error(dm[n][i], ref) / (FACTOR * fl[what]) for n in names}
                line.append(f"{what} floor {fl[what]:.2e} " + " ".join(f"{n} {v:.0f}x" for n, v in miss.items()))
            print(" | ".join(line), flush=True)
    wn = O.references((O.CUT_CASE, O.CUT_K))[torch.float64].wn
    print("cut-off case weights, sorted:", [round(float(v), 4) for v in wn.flatten().sort().values])


if __name__ == "__main__":
    main()
