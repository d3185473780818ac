"""Every existing unit's compiler input against the parent commit, and the resources of the row-select pull-back units: the
first tables of profiles/leapfrog_pull.txt.  No GPU needed.

    python scratch/leapfrog_pull_resources.py PARENT        (PARENT: git archive COMMIT | tar -x -C PARENT)

1. What the compiler is given for every translation unit both trees generate: the generated source, and every project header
   it includes, transitively (build.py's own ``_deps_hash``: the key of the object cache; ``load_build`` / ``inputs_of`` of
   scratch/pullback_resources.py).  Where both are the same bytes the object keeps its cache key; the others are listed.
2. The units only this tree generates, compiled with -Rpass-analysis=kernel-resource-usage: the compiler's own remarks on
   registers, scratch, spills and occupancy by registers, beside the pull-back unit of the same shape; and the dynamic LDS of a
   3 x 256 tile at K = 1 from the launcher's formula.
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from pullback_resources import ROOT, inputs_of            # noqa: E402

FIELDS = (("vgpr", "VGPRs"), ("agpr", "AGPRs"), ("sgpr", "TotalSGPRs"), ("scratch", "ScratchSize [bytes/lane]"),
          ("vspill", "VGPRs Spill"), ("sspill", "SGPRs Spill"), ("occupancy", "Occupancy [waves/SIMD]"))


def remarks(b, gen: Path, name: str, work: Path):
    """The kernel-resource-usage remarks of one generated unit."""
    cmd = [b._hipcc(), "-O3", "-std=c++17", "-fPIC", "-Wno-inline-asm", "-x", "hip", f"--offload-arch={b.ARCH}", f"-I{b.CSRC}",
           f"-I{b.ROOT / 'include'}", "-c", str(gen / f"{name}.hip"), "-o", str(work / f"{name}.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=work)
    assert r.returncode == 0, r.stderr
    return {f: int(re.search(re.escape(key) + r":\s*(\d+)", r.stderr).group(1)) for f, key in FIELDS}


def main(parent_root: Path):
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        _, P = inputs_of(parent_root, "parent_build", tmp / "parent_gen")
        b, T = inputs_of(ROOT, "this_build", tmp / "this_gen")
        gone, new = sorted(set(P) - set(T)), sorted(set(T) - set(P))
        assert not gone, f"units of the parent this tree does not generate: {gone}"
        same = [n for n in sorted(P) if P[n] == T[n]]
        other = [n for n in sorted(P) if P[n] != T[n]]
        print("# ---- the compiler's input, parent against this tree: generated source + every project header it includes ----")
        print(f"{len(P)} translation units in the parent ({sum(n.endswith('.hip') for n in P)} kernel units); identical input "
              f"(the object keeps its cache key): {len(same)}")
        print(f"input differs: {len(other)}")
        for n in other:
            what = [w for w, i in (("source", 0), ("headers", 1)) if P[n][i] != T[n][i]]
            print(f"    {n}: {' and '.join(what)} differ")
        print(f"units only this tree generates: {new}")
        print("\n# ---- the row-select pull-back units, each under the pull-back unit of its shape (the compiler's remarks) ----")
        print("# " + " ".join(f for f, _ in FIELDS) + "   (occupancy: by registers)")
        work = tmp / "work"
        work.mkdir()
        for n in new:
            name = n[:-4]
            for unit in (name.replace("mlp_pullsel_", "mlp_pull_"), name):
                m = remarks(b, tmp / "this_gen", unit, work)
                print(f"{unit:32s} " + " ".join(f"{m[f]:>9d}" for f, _ in FIELDS), flush=True)
        # dynamic LDS of one tile (ff_api.cpp pull_lds_bytes): slots x (dregs + cregs) x 256 bytes + (tile / (1 + K)) x n_hidden x width x 4
        print("\n# ---- dynamic LDS per tile at 3 x 256, K = 1, one stage slot (a leapfrog table names slot 0 only) ----")
        for tile, h, d, c, _, _ in b.PULL_SELECT_INSTANCES:
            lds = 1 * (d + c) * 256 + (tile // 2) * 3 * h * 4
            print(f"{b._pullsel_name(tile, h, d, c, 1, 0):32s} {lds:>7d} bytes ({lds / 1024:.1f} KiB; width {h} on chip)")


if __name__ == "__main__":
    main(Path(sys.argv[1]).resolve())
