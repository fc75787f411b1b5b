"""The Julia binding's heatbath extends the Gaugefields generics the reference's Heatbath update calls (src/updates/heatbath.jl:27,36,39:
`Heatbath(U, β, ITERATION_MAX = ...)`, `heatbath!(U, hb)`, `overrelaxation!(U, hb)`), so update! dispatches to the device once the driver holds a
HIPHeatbath; an exported function of the same name would leave those calls on the package's host code.  Static: there is no Julia here."""
import os
import re

from conftest import ROOT

SRC = open(os.path.join(ROOT, "julia", "LatticeQCDHIP.jl")).read()


def _block(head):
    m = re.search(head + r"(.*?)\n(?=\S)", SRC, flags=re.S)
    assert m, head
    return set(re.findall(r"[A-Za-z_][\w!]*", m.group(1)))


def test_heatbath_methods_extend_the_gaugefields_generics():
    imported = _block(r"\nimport Gaugefields:")
    exported = _block(r"\nexport ")
    for name in ("Heatbath", "heatbath!", "overrelaxation!"):
        assert name in imported, f"{name} must be imported from Gaugefields and extended"
        assert name not in exported, f"{name} must not be exported as a function of its own"


def test_methods_on_the_device_links_exist():
    assert re.search(r"(?m)^Heatbath\(U::Vector\{HIPLink\}, β; ITERATION_MAX", SRC)
    assert re.search(r"(?m)^function heatbath!\(U::Vector\{HIPLink\}, hb::HIPHeatbath\)", SRC)
    assert re.search(r"(?m)^function overrelaxation!\(U::Vector\{HIPLink\}, hb::HIPHeatbath\)", SRC)


def test_the_ccalls_name_the_heatbath_entry_points():
    for sym in ("lqcd_gauge_heatbath", "lqcd_gauge_overrelax", "lqcd_gauge_heatbath_measure"):
        assert re.search(r"ccall\(\(:" + sym + r", LIB\)", SRC), sym
