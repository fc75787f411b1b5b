"""The Julia binding's multi-column entries: one ccall each of lqcd_op_hop_multi, lqcd_op_apply_multi and lqcd_solve_bicgstab_eo_multi behind hop_multi!,
mul_multi! and solve_DinvX_multi!, with the argument lists of the C prototypes, and the exports.  Static: there is no Julia here; that the types match the
header is checked by test_host_logic.py::test_julia_binding_matches_the_c_header."""
import os
import re

from conftest import ROOT

SRC = open(os.path.join(ROOT, "julia", "LatticeQCDHIP.jl"), encoding="utf-8").read()
HDR = open(os.path.join(ROOT, "include", "lqcd_hip.h"), encoding="utf-8").read()
COLS = r"\(ys::Vector\{HIPFermion\}, D::HIPDirac, xs::Vector\{HIPFermion\}\)"
HANDLES = r"D\.h, length\(ys\), \[y\.h for y in ys\], \[x\.h for x in xs\], D\.dagger"


def _body(name):
    m = re.search(r"(?ms)^function %s%s\n(.*?)^end" % (re.escape(name), COLS), SRC)
    assert m, f"{name}(ys, D, xs) is missing"
    return m.group(1)


def test_header_declares_the_three_entries_and_the_limit():
    assert re.search(r"(?m)^#define LQCD_MRHS_MAX 12$", HDR)
    for proto in (r"int lqcd_op_hop_multi\(lqcd_op_t op, int n, const lqcd_spinor_t\* out, const lqcd_spinor_t\* in, int dagger\);",
                  r"int lqcd_op_apply_multi\(lqcd_op_t op, int n, const lqcd_spinor_t\* out, const lqcd_spinor_t\* in, int dagger\);",
                  r"int lqcd_solve_bicgstab_eo_multi\(lqcd_op_t op, int n, const lqcd_spinor_t\* x, const lqcd_spinor_t\* b, int dagger,\s*"
                  r"double eps, int maxiter, int\* iters /\* \[n\] or NULL \*/, double\* final_rr /\* \[n\] or NULL \*/\);"):
        assert re.search(proto, HDR), proto
    for key in ("mrhs_active", "meson_mrhs"):
        assert key in HDR, key


def test_hop_multi_is_one_ccall():
    body = _body("hop_multi!")
    assert body.count("ccall") == 1
    assert re.search(r"ccall\(\(:lqcd_op_hop_multi, LIB\), Cint, \(Ptr\{Cvoid\}, Cint, Ptr\{Ptr\{Cvoid\}\}, Ptr\{Ptr\{Cvoid\}\}, Cint\),\s*" + HANDLES + r"\)", body)


def test_mul_multi_is_one_ccall():
    body = _body("mul_multi!")
    assert body.count("ccall") == 1
    assert re.search(r"ccall\(\(:lqcd_op_apply_multi, LIB\), Cint, \(Ptr\{Cvoid\}, Cint, Ptr\{Ptr\{Cvoid\}\}, Ptr\{Ptr\{Cvoid\}\}, Cint\),\s*" + HANDLES + r"\)", body)


def test_solve_multi_is_one_ccall_with_per_column_outputs():
    body = _body("solve_DinvX_multi!")
    assert body.count("ccall") == 1
    assert re.search(r"ccall\(\(:lqcd_solve_bicgstab_eo_multi, LIB\), Cint, "
                     r"\(Ptr\{Cvoid\}, Cint, Ptr\{Ptr\{Cvoid\}\}, Ptr\{Ptr\{Cvoid\}\}, Cint, Float64, Cint, Ptr\{Cint\}, Ptr\{Float64\}\),\s*"
                     + HANDLES + r", D\.eps_CG, D\.MaxCGstep, its, rrs\)", body)
    assert re.search(r"its, rrs = zeros\(Cint, length\(ys\)\), zeros\(Float64, length\(ys\)\)", body)
    assert 'D.method_CG == "bicgstab_evenodd"' in body


def test_exports():
    exported = re.search(r"\nexport (.*?)\n(?=\S)", SRC, flags=re.S).group(1)
    for name in ("hop_multi!", "mul_multi!", "solve_DinvX_multi!"):
        assert name in exported, name
