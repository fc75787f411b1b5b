"""The Julia binding reaches the five entries of the plaquette + rectangle action: calc_dSdUμ! and evaluate_GaugeAction of a GaugeAction that holds the
rectangle set (a second push! of the package's own) dispatch to the improved entries instead of raising, the fused forms and the rectangle mean are
wrapped.  Static: there is no Julia here."""
import os
import re

from conftest import ROOT

SRC = re.sub(r"(?m)#.*$", "", open(os.path.join(ROOT, "julia", "LatticeQCDHIP.jl")).read())


def _ccall(sym):
    m = re.search(r"ccall\(\(:" + sym + r", LIB\), Cint,\s*\(([^)]*)\)", SRC)
    assert m, sym
    return [t.strip() for t in m.group(1).split(",") if t.strip()]


def test_the_five_entries_are_wrapped_with_their_c_signatures():
    assert _ccall("lqcd_gauge_rectangle") == ["Ptr{Cvoid}", "Ref{Float64}"]
    assert _ccall("lqcd_gauge_action_improved") == ["Ptr{Cvoid}", "Float64", "Float64", "Ref{Float64}"]
    assert _ccall("lqcd_gauge_force_improved") == ["Ptr{Cvoid}", "Ptr{Cvoid}", "Float64", "Float64"]
    assert _ccall("lqcd_momentum_add_gauge_force_improved") == ["Ptr{Cvoid}", "Float64", "Ptr{Cvoid}", "Float64", "Float64"]
    assert _ccall("lqcd_link_staple_improved") == ["Ptr{Cvoid}", "Cint", "Ptr{Cvoid}", "Cint", "Float64", "Float64"]


def test_the_signatures_are_the_header_s():
    hdr = open(os.path.join(ROOT, "include", "lqcd_hip.h")).read()
    ctype = {"lqcd_gauge_t": "Ptr{Cvoid}", "double": "Float64", "double*": "Ref{Float64}", "int": "Cint"}
    for sym in ("lqcd_gauge_rectangle", "lqcd_gauge_action_improved", "lqcd_gauge_force_improved", "lqcd_momentum_add_gauge_force_improved",
                "lqcd_link_staple_improved"):
        m = re.search(r"\bint " + sym + r"\(([^)]*)\);", hdr)
        assert m, sym
        want = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).split(",")]
        assert _ccall(sym) == want, sym


def test_the_rectangle_set_is_accepted_not_refused():
    i = SRC.index("function betas_inp(ga::GaugeAction{4,HIPLink})")
    body = SRC[i:SRC.index("\nend", i)]
    assert "n == 12" in body and "n == 24" in body and "error(" in body            # plaquette set, rectangle set, anything else
    assert "implements the plaquette action" not in SRC
    assert re.search(r"(?m)^beta_inp\(ga::GaugeAction\{4,HIPLink\}\) = betas_inp\(ga\)\[1\]", SRC)
    assert re.search(r"(?m)^beta_rect_inp\(ga::GaugeAction\{4,HIPLink\}\) = betas_inp\(ga\)\[2\]", SRC)


def test_the_generics_dispatch_on_the_rectangle_coefficient():
    i = SRC.index("calc_dSdUμ!(dSdUμ::HIPLink, ga::GaugeAction{4,HIPLink}")
    body = SRC[i:i + re.search(r"\n(?=\S)", SRC[i:]).start()]
    assert "beta_rect_inp(ga) != 0 ? link_staple_improved!(dSdUμ, ga, μ, U)" in body and "lqcd_link_staple," in body
    i = SRC.index("link_staple_improved!(dSdUμ::HIPLink")
    body = SRC[i:i + re.search(r"\n(?=\S)", SRC[i:]).start()]
    assert "lqcd_link_staple_improved" in body and "2 * beta_inp(ga), 2 * beta_rect_inp(ga)" in body      # beta/2 is pushed on the loop and on its adjoint
    i = SRC.index("function evaluate_GaugeAction(ga::GaugeAction{4,HIPLink}")
    body = SRC[i:SRC.index("\nend", i)]
    assert "lqcd_gauge_action_improved" in body and "lqcd_gauge_action," in body and "2 * bp, 2 * br" in body and "return -3 * s[]" in body
    assert re.search(r"(?m)^P_update_fused!\(U::Vector\{HIPLink\}, p::Vector\{HIPTALink\}, factor, β_plaq, β_rect\) =", SRC)
    assert re.search(r"(?m)^function calculate_Rectangle\(U::Vector\{HIPLink\}\)", SRC)
    exported = SRC[SRC.index("\nexport "):SRC.index("\n\n", SRC.index("\nexport "))]
    assert "calculate_Rectangle" in exported and "gauge_force_improved!" in exported
