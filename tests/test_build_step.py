"""The one compile step (cgmres_cpp_amd/build.py compile()): its staleness rule on fabricated records, and a plugin whose
header includes a header of its own."""
import os
import shutil

import pytest

from cgmres_cpp_amd import build as B
from cgmres_cpp_amd import plugin

needs_hipcc = pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="hipcc not available")


def _touch(path, t, text=""):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    os.utime(path, (t, t))


def test_staleness_rule_on_fabricated_records(tmp_path, monkeypatch):
    """Nothing is built: an artefact, its source, an own header (recorded relative to the repository root) and a foreign
    header (recorded by absolute path), with chosen mtimes."""
    root, outside = str(tmp_path / "tree"), str(tmp_path / "outside" / "user.hpp")
    monkeypatch.setattr(B, "ROOT", root)
    src, hdr, out = (os.path.join(root, n) for n in ("csrc/a.hip", "csrc/a.h", "lib/a.so"))

    def lay(t_out=200, t_hdr=100, t_user=100, record=f"csrc/a.hip\ncsrc/a.h\n{outside}\n"):
        shutil.rmtree(root, ignore_errors=True)
        _touch(src, 100), _touch(hdr, t_hdr), _touch(outside, t_user), _touch(out, t_out)
        if record is not None:
            _touch(out + ".d", t_out, record)

    lay()
    assert B.read_deps(out) == [src, hdr, outside]
    assert not B.needs_compile(out, src)
    lay(t_hdr=200)  # as old as the artefact: still kept
    assert not B.needs_compile(out, src)
    lay(t_hdr=201)
    assert B.needs_compile(out, src)
    lay(t_user=201)
    assert B.needs_compile(out, src)
    lay(record=None)
    assert B.needs_compile(out, src)
    lay()
    os.remove(hdr)
    assert B.needs_compile(out, src)
    lay()
    os.remove(out)
    assert B.needs_compile(out, src)
    # the tree moves, artefacts and records with it (mtimes kept): the record's relative names follow it
    lay()
    moved = str(tmp_path / "elsewhere")
    shutil.copytree(root, moved, copy_function=shutil.copy2)
    shutil.rmtree(root)
    monkeypatch.setattr(B, "ROOT", moved)
    m_src, m_out = os.path.join(moved, "csrc/a.hip"), os.path.join(moved, "lib/a.so")
    assert B.read_deps(m_out) == [m_src, os.path.join(moved, "csrc/a.h"), outside]
    assert not B.needs_compile(m_out, m_src)
    os.utime(os.path.join(moved, "csrc/a.h"), (201, 201))
    assert B.needs_compile(m_out, m_src)


@needs_hipcc
def test_plugin_rebuilds_when_a_nested_header_changes(tmp_path):
    """An operator header that includes a second header: the record of the build names both, so the plugin is kept while
    neither changes and rebuilt when the nested one does."""
    user = tmp_path / "user dir"  # (a blank in the path: the compiler's rule escapes it, the record must not)
    user.mkdir()
    inner, outer = user / "coeffs.hpp", user / "nested_op.hpp"
    inner.write_text("constexpr double kDiag = 2.5;\n")
    outer.write_text('#include "coeffs.hpp"\n'
                     "struct NestedOp {\n"
                     "  static constexpr int len = 8, n_params = 0;\n"
                     "  static double Ax_row(int i, const double* x, const double*) { return kDiag * x[i]; }\n"
                     "};\n")
    name = "nested_include_test"
    try:
        out = plugin.build_operator(str(outer), "NestedOp", name=name)
        deps = B.read_deps(out)
        assert os.path.realpath(inner) in deps and os.path.realpath(outer) in deps
        assert os.path.join(B.CSRC, "user_operator.hip.h") in deps
        before = os.stat(out).st_mtime_ns
        assert plugin.build_operator(str(outer), "NestedOp", name=name) == out
        assert os.stat(out).st_mtime_ns == before
        later = os.path.getmtime(out) + 10
        os.utime(inner, (later, later))
        plugin.build_operator(str(outer), "NestedOp", name=name)
        assert os.stat(out).st_mtime_ns != before
    finally:
        for f in (f"libcgmres_op_{name}.so", f"libcgmres_op_{name}.so.d", f"op_{name}.hip"):
            if os.path.exists(os.path.join(plugin.PLUGIN_DIR, f)):
                os.remove(os.path.join(plugin.PLUGIN_DIR, f))


@needs_hipcc
def test_operator_isa_summary_uses_the_plugin_template(tmp_path):
    """tools/isa_summary.py --operator formats plugin.TEMPLATE itself: it must keep up with the template's fields."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "isa_summary.py"), "--operator",
                        os.path.join(root, "tests", "user_models", "gmres_row_ops.hpp"), "SpdTridiagRowOp"],
                       env=dict(os.environ, ISA_TMP=str(tmp_path)), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "gmres_wave_kernel<SpdTridiagRowOp>" in r.stdout
