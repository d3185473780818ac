"""Every existing unit's compiler input against the parent commit, and the resources of the row-select push-forward units: the
first tables of profiles/leapfrog_push.txt.  No GPU needed.

    python scratch/leapfrog_push_resources.py PARENT        (PARENT: git archive COMMIT | tar -x -C PARENT)

1. What the compiler is given for every translation unit both trees generate: the generated source, and every project header
   it includes, transitively (build.py's own ``_deps_hash``: the key of the object cache; ``load_build`` / ``inputs_of`` of
   scratch/pullback_resources.py).  Where both are the same bytes the object keeps its cache key; the others are listed.
2. The units only this tree generates, compiled with -Rpass-analysis=kernel-resource-usage: the compiler's own remarks on
   registers, scratch, spills and occupancy by registers, beside the push-forward unit of the same shape.
"""
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from pullback_resources import ROOT, inputs_of            # noqa: E402
from leapfrog_pull_resources import FIELDS, remarks       # noqa: E402


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
        print("\n# ---- the row-select push-forward units, each under the push-forward unit of its shape (the compiler's remarks) ----")
        print("# " + " ".join(f for f, _ in FIELDS) + "   (occupancy: by registers)")
        work = tmp / "work"
        work.mkdir()
        for n in new:
            name = n[:-4]
            for unit in (name.replace("mlp_pushsel_", "mlp_push_"), name):
                m = remarks(b, tmp / "this_gen", unit, work)
                print(f"{unit:32s} " + " ".join(f"{m[f]:>9d}" for f, _ in FIELDS), flush=True)


if __name__ == "__main__":
    main(Path(sys.argv[1]).resolve())
