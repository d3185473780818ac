"""Resources and instructions of every unit generated from ff_mlp_ode.hpp / ff_mlp_pair.hpp, the parent commit against
this tree with its push-forward units: the tables of profiles/pushforward_resources.txt.  No GPU needed.

    python scratch/hutch_probe_out_resources.py measure PARENT parent.json       (PARENT: git archive COMMIT | tar -x -C PARENT)
    python scratch/hutch_probe_out_resources.py measure . this.json
    python scratch/pushforward_resources.py parent.json this.json

`measure` is scratch/hutch_probe_out_resources.py's.  This report takes two measurements whose unit lists differ: the units
both trees generate are compared figure by figure and instruction by instruction, the units only this tree generates (the
push-forward family) are listed beside the Hutchinson unit of the same shape.
"""
import json
import sys
from pathlib import Path

FIELDS = ("vgpr", "agpr", "sgpr", "scratch", "vspill", "sspill", "lds", "occupancy", "mfma")


def _insts(json_path: Path, name: str):
    lines = (Path(str(json_path) + ".asm") / f"{name}.isa").read_text().splitlines()
    return [l for l in lines if not l.startswith(("-", "amdhsa"))]


def report(parent: Path, this: Path) -> None:
    P, T = json.loads(parent.read_text()), json.loads(this.read_text())
    gone, new = sorted(set(P) - set(T)), sorted(set(T) - set(P))
    assert not gone, f"units of the parent this tree does not generate: {gone}"
    print("# ---- resources: parent / this, every unit both trees generate ----")
    print("# " + " ".join(f"{f}(parent/this)" for f in FIELDS))
    moved = []
    for name in sorted(P):
        cells = [f"{P[name][f]}/{T[name][f]}" for f in FIELDS]
        moved += [(name, f, P[name][f], T[name][f]) for f in FIELDS if P[name][f] != T[name][f]]
        print(f"{name:44s} " + " ".join(f"{c:>11s}" for c in cells))
    print(f"\n{len(P)} units; figures that differ from the parent's: {moved if moved else 'none'}")
    print("\n# ---- instructions: parent against this ----")
    same, other = [], []
    for name in sorted(P):
        a, b = _insts(parent, name), _insts(this, name)
        d = [(x, y) for x, y in zip(a, b) if x != y]
        (same if len(a) == len(b) and not d else other).append((name, len(a), len(b), d))
    print(f"{len(P)} units, {sum(len(_insts(parent, n)) for n in P)} instructions in all.")
    print(f"identical, instruction for instruction: {len(same)} units")
    print(f"not identical: {len(other)} units; their differing instructions (parent -> this):")
    for name, la, lb, d in other:
        print(f"    {name:40s} {la} / {lb} instructions, {len(d)} differ" +
              "".join(f"\n        {x:44s} -> {y}" for x, y in d[:4]))
    print("\n# ---- the push-forward units (this tree only), each under the Hutchinson unit of its shape ----")
    print("# " + " ".join(FIELDS) + " instructions")
    for name in new:
        twin = name.replace("mlp_push_", "mlp_ode_").replace("_w", "_t1_w")
        for n in (twin, name):
            if n in T:
                print(f"{n:44s} " + " ".join(f"{T[n][f]:>9d}" for f in FIELDS) + f" {len(_insts(this, n)):>9d}")


if __name__ == "__main__":
    report(Path(sys.argv[1]), Path(sys.argv[2]))
