"""The Julia binding's Wilson loops: one ccall of lqcd_gauge_wilson_loops behind wilson_loops(U, Rmax, Tmax), and calc_Wilson_loop with the reference's
argument order (src/measurements/measure_Wilsonloop.jl:71: calc_Wilson_loop(U, Lt, Ls), the time extent first).  Static: there is no Julia here; the
prototype itself is checked by test_host_logic.py::test_julia_binding_matches_the_c_header."""
import os
import re

from conftest import ROOT

SRC = open(os.path.join(ROOT, "julia", "LatticeQCDHIP.jl"), encoding="utf-8").read()


def test_wilson_loops_is_one_ccall_and_returns_rmax_by_tmax():
    m = re.search(r"(?ms)^function wilson_loops\(U::Vector\{HIPLink\}, Rmax::Integer, Tmax::Integer\)\n(.*?)^end", SRC)
    assert m, "wilson_loops(U::Vector{HIPLink}, Rmax, Tmax) is missing"
    body = m.group(1)
    assert body.count("ccall") == 1 and re.search(r"ccall\(\(:lqcd_gauge_wilson_loops, LIB\), Cint, \(Ptr\{Cvoid\}, Cint, Cint, Ptr\{Float64\}\), whole\(U\)\.h, Rmax, Tmax, \w+\)", body)
    # the C table is row-major [Rmax][Tmax]: a column-major Tmax x Rmax buffer, read back transposed
    assert re.search(r"zeros\(Float64, Tmax, Rmax\)", body)
    assert re.search(r"\[(\w+)\[t, r\] for r = 1:Rmax, t = 1:Tmax\]", body)


def test_calc_wilson_loop_takes_the_time_extent_first():
    m = re.search(r"(?m)^calc_Wilson_loop\(U::Vector\{HIPLink\}, Lt, Ls\) = (.*)$", SRC)
    assert m, "calc_Wilson_loop(U::Vector{HIPLink}, Lt, Ls) is missing"
    assert m.group(1).strip() == "wilson_loops(U, Ls, Lt)[Ls, Lt]"
    exported = re.search(r"\nexport (.*?)\n(?=\S)", SRC, flags=re.S).group(1)
    assert "wilson_loops" in exported and "calc_Wilson_loop" in exported
