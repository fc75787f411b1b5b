"""The Julia binding's meson correlators: one ccall of lqcd_meson_correlators behind meson_correlators(D, src) and one of lqcd_pion_correlator behind
pion_correlator(D, src), the table buffer transposed the right way, the Pion_correlator_measurement / measure pair, the exports.  Static: there is no Julia
here; the prototypes themselves are checked by test_host_logic.py::test_julia_binding_matches_the_c_header."""
import os
import re

from conftest import ROOT

SRC = open(os.path.join(ROOT, "julia", "LatticeQCDHIP.jl"), encoding="utf-8").read()


def _body(name):
    m = re.search(r"(?ms)^function %s\(D::HIPDirac, src = \(0, 0, 0, 0\)\)\n(.*?)^end" % name, SRC)
    assert m, f"{name}(D::HIPDirac, src) is missing"
    return m.group(1)


def test_meson_correlators_is_one_ccall_and_returns_16_by_glt():
    body = _body("meson_correlators")
    assert body.count("ccall") == 1
    assert re.search(r"ccall\(\(:lqcd_meson_correlators, LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cint\}, Float64, Cint, Ptr\{Float64\}, Ptr\{Cint\}\),\s*"
                     r"D\.h, Cint\[src\.\.\.\], D\.eps_CG, D\.MaxCGstep, \w+, C_NULL\)", body)
    # the C table is row-major [16][gLt]: a column-major gLt x 16 buffer, read back transposed
    assert re.search(r"zeros\(Float64, gLt, 16\)", body)
    assert re.search(r"\[(\w+)\[t, n\] for n = 1:16, t = 1:gLt\]", body)
    assert re.search(r"gLt = lattice\(D\.U\)\.L\[4\]", body)


def test_pion_correlator_is_one_ccall_of_glt_values():
    body = _body("pion_correlator")
    assert body.count("ccall") == 1
    assert re.search(r"ccall\(\(:lqcd_pion_correlator, LIB\), Cint, \(Ptr\{Cvoid\}, Ptr\{Cint\}, Float64, Cint, Ptr\{Float64\}, Ptr\{Cint\}\),\s*"
                     r"D\.h, Cint\[src\.\.\.\], D\.eps_CG, D\.MaxCGstep, \w+, C_NULL\)", body)
    assert re.search(r"zeros\(Float64, lattice\(D\.U\)\.L\[4\]\)", body)


def test_measurement_pair_and_exports():
    assert re.search(r"(?m)^struct Pion_correlator_measurement\n", SRC)
    m = re.search(r"(?m)^measure\(m::Pion_correlator_measurement, U::Vector\{HIPLink\}\) = (.*)$", SRC)
    assert m and m.group(1).strip() == "pion_correlator(m.D(U))"
    # the reference's constructor defaults (measure_Pion_correlator.jl:14-29)
    ctor = re.search(r"(?s)function Pion_correlator_measurement\(U::Vector\{HIPLink\};(.*?)\)\n", SRC).group(1)
    for kw in ('fermiontype = "Staggered"', "mass = 0.1", "Nf = 2", "κ = 1", "r = 1", "eps_CG = 1e-14", "MaxCGstep = 3000", "BoundaryCondition = nothing"):
        assert kw in ctor, kw
    exported = re.search(r"\nexport (.*?)\n(?=\S)", SRC, flags=re.S).group(1)
    for name in ("meson_correlators", "pion_correlator", "Pion_correlator_measurement", "measure"):
        assert name in exported, name
