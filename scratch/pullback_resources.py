"""Every existing unit against the parent commit, and the resources of the pull-back units: the tables of
profiles/pullback_resources.txt.  No GPU needed.

    python scratch/pullback_resources.py PARENT        (PARENT: git archive COMMIT | tar -x -C PARENT)

1. What the compiler is given for every translation unit both trees generate: the generated source, and every project
   header it includes, transitively (build.py's own ``_deps_hash``: the key of the object cache).  Where both are the same
   bytes, the same compiler with the same flags emits the same instructions; a unit whose input differs
   is listed; the kernel units among them are compiled from both trees and compared instruction by instruction.
2. The units only this tree generates (the pull-back family), compiled here with -Rpass-analysis=kernel-resource-usage and
   -save-temps: registers, scratch, spills, occupancy by registers, MFMA and instruction counts, beside the push-forward
   unit of the same shape.
"""
import importlib.util
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def load_build(root: Path, name: str):
    spec = importlib.util.spec_from_file_location(name, root / "flowfusion_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def inputs_of(root: Path, name: str, gen: Path):
    b = load_build(root, name)
    out = {}
    for src in b._gen_sources(gen):
        out[src.name] = (src.read_bytes(), b._deps_hash(src))
    return b, out


def measure(b, gen: Path, name: str, work: Path):
    src = gen / f"{name}.hip"
    cmd = [b._hipcc(), "-O3", "-std=c++17", "-fPIC", "-Wno-inline-asm", "-x", "hip", f"--offload-arch={b.ARCH}", f"-I{b.CSRC}",
           f"-I{b.ROOT / 'include'}", "-c", str(src), "-o", str(work / f"{name}.o"), "-save-temps=obj",
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=work)
    assert r.returncode == 0, r.stderr
    get = lambda key: int(re.search(re.escape(key) + r":\s*(\d+)", r.stderr).group(1))
    asm = next(work.glob(f"{name}-hip-amdgcn-*.s")).read_text().splitlines()
    body = [l.strip() for l in asm if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    return dict(vgpr=get("VGPRs"), agpr=get("AGPRs"), sgpr=get("TotalSGPRs"), scratch=get("ScratchSize [bytes/lane]"),
                vspill=get("VGPRs Spill"), sspill=get("SGPRs Spill"), occupancy=get("Occupancy [waves/SIMD]"),
                mfma=sum(l.startswith("v_mfma") for l in body), instructions=len(body))


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
        print(f"{len(P)} translation units in the parent ({sum(n.endswith('.hip') for n in P)} kernel units); identical input: {len(same)}")
        print(f"input differs: {len(other)}: {other}")
        for n in other:
            what = [w for w, i in (("source", 0), ("headers", 1)) if P[n][i] != T[n][i]]
            print(f"    {n}: {' and '.join(what)} differ")
        # a unit whose input differs only by the public header's new declarations: compile both, compare the device code
        for n in other:
            if not n.endswith(".hip"):
                continue
            isa = []
            for root, bb in ((parent_root, sys.modules["parent_build"]), (ROOT, b)):
                r = subprocess.run([bb._hipcc(), "-O3", "-std=c++17", "-fPIC", "-Wno-inline-asm", "-x", "hip", f"--offload-arch={bb.ARCH}",
                                    "--cuda-device-only", "-S", f"-I{bb.CSRC}", f"-I{bb.ROOT / 'include'}", str(bb.CSRC / n), "-o", "-"],
                                   capture_output=True, text=True)
                assert r.returncode == 0, r.stderr
                isa.append([l.strip() for l in r.stdout.splitlines() if l.startswith("\t") and not l.strip().startswith((".", ";"))])
            print(f"    {n}: {len(isa[0])} / {len(isa[1])} device instructions, "
                  f"{'identical, instruction for instruction' if isa[0] == isa[1] else 'DIFFERENT'}", flush=True)
        print(f"units only this tree generates: {new}")
        print("\n# ---- the pull-back units, each under the push-forward unit of its shape ----")
        fields = ("vgpr", "agpr", "sgpr", "scratch", "vspill", "sspill", "occupancy", "mfma", "instructions")
        print("# " + " ".join(fields) + "   (occupancy: by registers; the LDS stash bounds it further, profiles/pullback.txt)")
        work = tmp / "work"
        work.mkdir()
        for n in new:
            if not n.startswith("mlp_pull_"):
                continue
            name = n[:-4]
            twin = next(p[:-4] for p in T if p.startswith(name.replace("mlp_pull_", "mlp_push_")))
            for unit in (twin, name):
                m = measure(b, tmp / "this_gen", unit, work)
                print(f"{unit:32s} " + " ".join(f"{m[f]:>9d}" for f in fields), flush=True)


if __name__ == "__main__":
    main(Path(sys.argv[1]).resolve())
