"""tools/kernel_diff.py on assembly snippets: a kernel renumbered by one added
in front of it is identical; a changed instruction, a changed resource figure
and a kernel only one side has are each reported, with exit status 1.  With
--renames a kernel pairs with its renamed self; a map line that names no kernel
of the first file, or shares its old or new symbol with another, is exit status
2."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_diff.py")


def kernel(name, n, body="\tv_add_u32 v1, v0, v0\n", sgpr=16):
    """Kernel `name` as the n-th function of its file."""
    return (f"{name}:\n\ts_cbranch_scc1 .LBB{n}_2 ; a comment\n{body}.LBB{n}_2:\n\ts_endpgm\n"
            f".Lfunc_end{n}:\n"
            f"\t.amdhsa_kernel {name}\n\t\t.amdhsa_next_free_vgpr 8\n"
            f"\t\t.amdhsa_next_free_sgpr {sgpr}\n\t\t.amdhsa_kernarg_size 64\n"
            f"\t.end_amdhsa_kernel\n")


def run(tmp_path, a, b):
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    pa.write_text(a)
    pb.write_text(b)
    r = subprocess.run([sys.executable, TOOL, str(pa), str(pb)], capture_output=True, text=True)
    return r.returncode, r.stdout


def test_renumbered_kernels_are_identical(tmp_path):
    rc, out = run(tmp_path, kernel("_Zone", 0) + kernel("_Ztwo", 1),
                  kernel("_Ztwo", 0) + kernel("_Zone", 1))
    assert rc == 0, out
    assert "2 of 2 common kernels identical" in out


def test_differences_are_reported(tmp_path):
    base = kernel("_Zone", 0) + kernel("_Ztwo", 1) + kernel("_Zthree", 2)
    other = (kernel("_Zone", 0, body="\tv_add_u32 v1, v0, v1\n") + kernel("_Ztwo", 1, sgpr=24)
             + kernel("_Zfour", 2))
    rc, out = run(tmp_path, base, other)
    assert rc == 1
    lines = out.splitlines()
    assert lines[lines.index("instruction streams differ: 1") + 1].strip() == "_Zone"
    assert lines[lines.index("resources differ: 1") + 1].strip() == "_Ztwo"
    assert "next_free_sgpr 16 -> 24" in out
    assert any(l.startswith("only in") and l.endswith("a.s: 1") for l in lines)
    assert "  _Zthree" in lines and "  _Zfour" in lines


def run_renamed(tmp_path, a, b, renames):
    """As run(), with `renames` ("old new" lines) given as --renames."""
    pa, pb, pm = tmp_path / "a.s", tmp_path / "b.s", tmp_path / "map.txt"
    pa.write_text(a)
    pb.write_text(b)
    pm.write_text(renames)
    r = subprocess.run([sys.executable, TOOL, "--renames", str(pm), str(pa), str(pb)],
                       capture_output=True, text=True)
    return r.returncode, r.stdout, r.stderr


def test_renamed_kernel_pairs_as_identical(tmp_path):
    # (a directive inside the stream names the kernel's own symbol)
    body = "\tv_add_u32 v1, v0, v0\n\t.type {0},@function\n"
    rc, out, _ = run_renamed(tmp_path,
                             kernel("_Zold", 0, body=body.format("_Zold")) + kernel("_Ztwo", 1),
                             kernel("_Ztwo", 0) + kernel("_Znew", 1, body=body.format("_Znew")),
                             "_Zold _Znew\n")
    assert rc == 0, out
    lines = out.splitlines()
    assert any(l.startswith("only in") and l.endswith("a.s: 0") for l in lines)
    assert any(l.startswith("only in") and l.endswith("b.s: 0") for l in lines)
    assert "2 of 2 common kernels identical" in out


def test_rename_to_a_different_body_is_a_stream_difference(tmp_path):
    rc, out, _ = run_renamed(tmp_path, kernel("_Zold", 0) + kernel("_Ztwo", 1),
                             kernel("_Znew", 0, body="\tv_add_u32 v1, v0, v1\n")
                             + kernel("_Ztwo", 1), "_Zold _Znew\n")
    assert rc == 1
    lines = out.splitlines()
    assert lines[lines.index("instruction streams differ: 1") + 1].strip() == "_Znew"
    assert "1 of 2 common kernels identical" in out


def test_unknown_old_and_duplicate_new_exit_2(tmp_path):
    a = kernel("_Zone", 0) + kernel("_Ztwo", 1)
    b = kernel("_Znew", 0) + kernel("_Ztwo", 1)
    rc, _, err = run_renamed(tmp_path, a, b, "_Zgone _Znew\n")
    assert rc == 2
    assert "_Zgone" in err and "not a kernel" in err
    rc, _, err = run_renamed(tmp_path, a, b, "_Zone _Znew\n_Ztwo _Znew\n")
    assert rc == 2
    assert "_Znew" in err
    rc, _, err = run_renamed(tmp_path, a, b, "_Zone _Znew\n_Zone _Zother\n")
    assert rc == 2
    assert "_Zone" in err
    # onto a kernel of the first file that keeps its name: the two would merge
    rc, _, err = run_renamed(tmp_path, a, b, "_Zone _Ztwo\n")
    assert rc == 2
    assert "_Ztwo" in err
