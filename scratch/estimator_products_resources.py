"""Resources of the three products units (mlp_vjp_kernel, csrc/ff_mlp_vjp.hpp), each under the pull-back unit it is the sibling
of: the table of profiles/estimator_products_resources.txt.  No GPU needed.

    python scratch/estimator_products_resources.py
"""
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "scratch"))
from pullback_resources import load_build, measure  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        b = load_build(ROOT, "this_build")
        b._gen_sources(tmp / "gen")
        fields = ("vgpr", "agpr", "sgpr", "scratch", "vspill", "sspill", "occupancy", "mfma", "instructions")
        print("# ---- the products units, each under the pull-back unit of its shape ----")
        print("# " + " ".join(fields) + "   (occupancy: by registers; the LDS stash bounds it further)")
        work = tmp / "work"
        work.mkdir()
        for inst in b.PULL_INSTANCES:
            for unit in (b._pull_name(*inst), b._vjp_name(*inst)):
                m = measure(b, tmp / "gen", unit, work)
                print(f"{unit:32s} " + " ".join(f"{m[f]:>9d}" for f in fields), flush=True)


if __name__ == "__main__":
    main()
