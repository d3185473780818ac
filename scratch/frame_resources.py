"""Kernel resources of every product translation unit generated from ff_mlp_ode.hpp / ff_mlp_pair.hpp.

    python scratch/frame_resources.py measure TREE OUT.json     # compile TREE's units to assembly, read the metadata
    python scratch/frame_resources.py table PARENT.json THIS.json > profiles/frame_resources.txt

`measure` compiles each unit of TREE's `build._gen_sources()` for the device only (no GPU needed):
    hipcc -O3 -std=c++17 -x hip --offload-arch=gfx950 --cuda-device-only -S -I<csrc> -I<include> unit.hip -o unit.s
and reads the kernel's .vgpr_count / .sgpr_count / .private_segment_fixed_size (scratch) / .vgpr_spill_count /
.sgpr_spill_count (SGPRs kept in VGPR lanes) / .group_segment_fixed_size (static LDS) from the metadata, "; NumAgprs:" and
"; Occupancy:" from the kernel's resource comment, and counts the v_mfma instructions.  TREE is a checkout of the commit to measure.
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
    tmp = Path(tempfile.mkdtemp(prefix="frame_res_"))
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
        asm.unlink()
        print(src.stem, r, flush=True)
        return src.stem, r

    order = sorted(units, key=lambda s: -B._cost(s))
    with ThreadPoolExecutor(max_workers=8) as ex:
        res = dict(ex.map(one, order))
    out.write_text(json.dumps(res, indent=1, sort_keys=True))


def table(parent: Path, this: Path) -> None:
    p, t = json.loads(parent.read_text()), json.loads(this.read_text())
    assert sorted(p) == sorted(t), "the two commits generate different units"
    print("# " + " ".join(f"{f}(parent/this)" for f in FIELDS))
    worse = []
    for name in sorted(p):
        cells = []
        for f in FIELDS:
            cells.append(f"{p[name][f]}/{t[name][f]}")
            up = t[name][f] < p[name][f] if f == "occupancy" else t[name][f] > p[name][f]
            if up:
                worse.append((name, f))
        print(f"{name:44s} " + " ".join(f"{c:>11s}" for c in cells))
    named = [w for w in worse if w[1] != "sspill"]
    print(f"\n{len(p)} units; worse than the parent in a figure the issue names: {named if named else 'none'}")
    print(f"more SGPRs in VGPR lanes than the parent: {sorted(w[0] for w in worse if w[1] == 'sspill') or 'none'}")


if __name__ == "__main__":
    if sys.argv[1] == "measure":
        measure(Path(sys.argv[2]).resolve(), Path(sys.argv[3]))
    else:
        table(Path(sys.argv[2]), Path(sys.argv[3]))
