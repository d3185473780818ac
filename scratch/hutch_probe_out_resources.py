"""Resources and instructions of every unit generated from ff_mlp_ode.hpp / ff_mlp_pair.hpp, a parent commit against this
tree: the tables of profiles/hutch_probe_out.txt.  No GPU needed.

    python scratch/hutch_probe_out_resources.py measure TREE OUT.json
    python scratch/hutch_probe_out_resources.py report PARENT.json THIS.json [FIRST_FORM.json]

`measure` is scratch/frame_resources.py's (same compile line, same figures) and also keeps each unit's instruction text
-- the assembly with comments, directives, labels and metadata taken out -- under OUT.json.asm/.  `report` prints the
resource table with its summary, the units on which the optional third measurement (another form of the change, here
the epilogue whose tangent lanes store their own column) moved a figure, and the instruction-by-instruction comparison of
the units without tangent columns.  TREE is a checkout of the commit to measure (git archive COMMIT | tar -x -C TREE).
The figures quoted for the other rejected forms are `measure`'s for the units named there, with the epilogue edited by hand.
"""
import json
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

FIELDS = ("vgpr", "agpr", "sgpr", "scratch", "vspill", "sspill", "lds", "occupancy", "mfma")


def measure(tree: Path, out: Path) -> None:
    sys.path.insert(0, str(tree))
    from flowfusion_amd import build as B
    tmp = Path(tempfile.mkdtemp(prefix="probe_out_res_"))
    keep = Path(str(out) + ".asm")
    keep.mkdir(exist_ok=True)
    units = [s for s in B._gen_sources(tmp / "gen") if s.suffix == ".hip" and
             re.search(r'#include "ff_mlp_(ode|pair)\.hpp"', s.read_text())]

    def one(src: Path):
        asm = tmp / (src.stem + ".s")
        subprocess.run([B._hipcc(), "-O3", "-std=c++17", "-x", "hip", f"--offload-arch={B.ARCH}", "--cuda-device-only", "-S",
                        "-Wno-inline-asm", f"-I{B.CSRC}", f"-I{B.ROOT / 'include'}", str(src), "-o", str(asm)], check=True)
        text = asm.read_text()
        meta = lambda key: int(re.search(rf"^\s*\.{key}:\s*(\d+)", text, re.M).group(1))
        note = lambda key: int(re.search(rf"^; {key}: (\d+)", text, re.M).group(1))
        r = dict(vgpr=meta("vgpr_count"), agpr=note("NumAgprs"), sgpr=meta("sgpr_count"),
                 scratch=meta("private_segment_fixed_size"), vspill=meta("vgpr_spill_count"), sspill=meta("sgpr_spill_count"),
                 lds=meta("group_segment_fixed_size"), occupancy=note("Occupancy"),
                 mfma=len(re.findall(r"^\s*v_mfma", text, re.M)))
        isa = [re.sub(r"\s*;.*$", "", l).strip() for l in text.splitlines()]
        isa = [l for l in isa if l and not l.startswith((".", ";", "//", "-", "amdhsa")) and not l.endswith(":")]
        (keep / (src.stem + ".isa")).write_text("\n".join(isa))
        asm.unlink()
        print(src.stem, r, flush=True)
        return src.stem, r

    order = sorted(units, key=lambda s: -B._cost(s))
    with ThreadPoolExecutor(max_workers=8) as ex:
        res = dict(ex.map(one, order))
    out.write_text(json.dumps(res, indent=1, sort_keys=True))


def _insts(json_path: Path, name: str):
    lines = (Path(str(json_path) + ".asm") / f"{name}.isa").read_text().splitlines()
    return [l for l in lines if not l.startswith(("-", "amdhsa"))]


def report(parent: Path, this: Path, first: Path = None) -> None:
    P, T = json.loads(parent.read_text()), json.loads(this.read_text())
    assert sorted(P) == sorted(T), "the two commits generate different units"
    tang = sorted(n for n in P if "_t1" in n)
    rest = sorted(n for n in P if "_t1" not in n)
    print("# ---- resources: parent / this, every unit generated from ff_mlp_ode.hpp / ff_mlp_pair.hpp ----")
    print("# " + " ".join(f"{f}(parent/this)" for f in FIELDS))
    worse = []
    for name in sorted(P):
        cells = []
        for f in FIELDS:
            cells.append(f"{P[name][f]}/{T[name][f]}")
            if (T[name][f] < P[name][f]) if f == "occupancy" else (T[name][f] > P[name][f]):
                worse.append((name, f))
        print(f"{name:44s} " + " ".join(f"{c:>11s}" for c in cells))
    named = [x for x in worse if x[1] != "sspill"]
    print(f"\n{len(P)} units ({len(tang)} tangent instantiations); a figure other than sspill above the parent's "
          f"(occupancy: below): {named if named else 'none'}")
    moved = sorted(n for n in P if P[n]["sspill"] != T[n]["sspill"])
    print(f"sspill differs on {len(moved)} units{', all tangent' if all('_t1' in n for n in moved) else ''}: " +
          ", ".join(f"{n.replace('mlp_ode_', '')} {P[n]['sspill']}->{T[n]['sspill']}" for n in moved))
    if first is not None:
        F = json.loads(first.read_text())
        cols = ("vgpr", "agpr", "scratch", "vspill", "sspill", "occupancy")
        print("\n# ---- the first form (tangent lanes sum and store; role - 1 as the index): parent / first form, "
              "units where a figure moved ----")
        print("# unit  " + "  ".join(cols))
        for name in tang:
            if any(P[name][f] != F[name][f] for f in cols if f != "sspill"):
                print(f"{name:44s} " + " ".join(f"{P[name][f]}/{F[name][f]:<6}" for f in cols))
        up = [n for n in tang if F[n]["vgpr"] > P[n]["vgpr"]]
        print(f"\nVGPRs above the parent's on {len(up)} tangent units (+{min(F[n]['vgpr'] - P[n]['vgpr'] for n in up)} .. "
              f"+{max(F[n]['vgpr'] - P[n]['vgpr'] for n in up)}), scratch on {sum(F[n]['scratch'] > P[n]['scratch'] for n in tang)}")
    print("\n# ---- instructions of the units without tangent columns (state-only, pair, row-select): parent against this ----")
    same, other = [], []
    for name in rest:
        a, b = _insts(parent, name), _insts(this, name)
        d = [(x, y) for x, y in zip(a, b) if x != y]
        (same if len(a) == len(b) and not d else other).append((name, len(a), len(b), d))
    print(f"{len(rest)} units, {sum(len(_insts(parent, n)) for n in rest)} instructions in all.")
    print(f"identical, instruction for instruction: {len(same)} units")
    print(f"not identical: {len(other)} units; their differing instructions (parent -> this):")
    for name, la, lb, d in other:
        print(f"    {name:40s} {la} / {lb} instructions, {len(d)} differ" +
              "".join(f"\n        {x:44s} -> {y}" for x, y in d[:4]))


if __name__ == "__main__":
    if sys.argv[1] == "measure":
        measure(Path(sys.argv[2]).resolve(), Path(sys.argv[3]))
    else:
        report(*[Path(a) for a in sys.argv[2:5]])
