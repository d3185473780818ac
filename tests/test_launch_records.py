"""What the C ABI enqueues, recorded without a GPU and compared with a committed record.

ff_api.cpp calls no HIP function itself: it plans, validates, sizes and then calls the `launch_<kernel>` functions the
generated ff_table.cpp declares.  Here those declarations are replaced by definitions that print their arguments, and
tests/launch_records/launch_records.cpp sweeps plans x batches x arguments x FF_COOP / FF_TAIL_SPLIT pins through the
public C ABI: launcher names, grids, LDS bytes, every KernelArgs field and the tail launch's pointer offsets, which only
the GPU tier exercises otherwise.

tests/launch_records/expected.txt is the driver's output built against the ff_api.cpp and table generator of the commit
BEFORE the launch path was folded into one launcher, never against the code under test.  A change that means to alter a
launch regenerates it from a tree it trusts:  python tests/test_launch_records.py <tree> > tests/launch_records/expected.txt
(`<tree>` a checkout of that commit; add --full for the text of every section when two trees have to be diffed).
"""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HERE = ROOT / "tests" / "launch_records"

_DECL = re.compile(r"^int (launch_\w+)\(const KernelArgs\*, unsigned, unsigned, hipStream_t\);$", re.M)
_PRELUDE = 'extern "C" int ff_test_record(const char*, const ff::KernelArgs*, unsigned, unsigned);\n'


def build_driver(tree: Path, work: Path, extra_flags=()) -> Path:
    """Compile `tree`'s ff_api.cpp, a recording copy of its generated kernel table and the driver into one host program."""
    sys.path.insert(0, str(tree))                  # (as a script: `tree`'s generator, not this checkout's)
    from flowfusion_amd import build as fb
    sys.path.pop(0)
    assert Path(fb.__file__).resolve().parents[1] == tree.resolve()
    gen = work / "gen"
    fb._gen_sources(gen=gen)
    table = (gen / "ff_table.cpp").read_text()
    assert len(_DECL.findall(table)) > 60
    table = _DECL.sub(r'int \1(const KernelArgs* a, unsigned g, unsigned l, hipStream_t) { return ff_test_record("\1", a, g, l); }', table)
    table = table.replace("namespace ff {\n", _PRELUDE + "namespace ff {\n", 1)
    assert "hipStream_t);" not in table            # no launcher left that would need the GPU
    rec = work / "ff_table_recording.cpp"
    rec.write_text(table)
    exe = work / "launch_records"
    hipcc = Path(fb._hipcc())
    cmd = [str(hipcc), "-O1", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__=1", f"-I{hipcc.resolve().parents[1] / 'include'}",
           f"-I{tree / 'flowfusion_amd' / 'csrc'}", f"-I{tree / 'include'}", *extra_flags,
           str(tree / "flowfusion_amd" / "csrc" / "ff_api.cpp"), str(rec), str(HERE / "launch_records.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return exe


def test_launches_match_the_recorded_ones(tmp_path):
    exe = build_driver(ROOT, tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got, want = r.stdout.splitlines(), (HERE / "expected.txt").read_text().splitlines()
    # the first line that differs names its section: run the driver with --full on both trees to see inside a digest
    section = ""
    for i, (g, w) in enumerate(zip(got, want)):
        if w.startswith("== "):
            section = w
        assert g == w, f"line {i + 1} of the record, in section {section!r}"
    assert len(got) == len(want)


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(Path(sys.argv[1]).resolve(), Path(tmp), [f for f in sys.argv[2:] if f.startswith("-f")])
        sys.exit(subprocess.run([str(exe)] + [f for f in sys.argv[2:] if f == "--full"]).returncode)
