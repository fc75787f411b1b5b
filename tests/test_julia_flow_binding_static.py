"""The Julia binding's gradient flow extends the Gaugefields generics the reference's driver imports (src/system/lqcd.jl:6-10: `import Gaugefields:
Gradientflow, flow!`), so `Gradientflow(univ.U, ...)` and `flow!(Usmr, gradientflow)` (lqcd.jl:99,153) dispatch to the device; a second, exported function
of the same name would leave the driver on the package's host flow.  `Usmr = deepcopy(univ.U)` (lqcd.jl:150) must copy the device field.  Static: there is
no Julia here."""
import os
import re

from conftest import ROOT

SRC = open(os.path.join(ROOT, "julia", "LatticeQCDHIP.jl")).read()


def _block(head):
    m = re.search(head + r"(.*?)\n(?=\S)", SRC, flags=re.S)
    assert m, head
    return set(re.findall(r"[A-Za-z_][\w!]*", m.group(1)))


def test_flow_methods_extend_the_gaugefields_generics():
    imported = _block(r"\nimport Gaugefields:")
    exported = _block(r"\nexport ")
    for name in ("Gradientflow", "flow!"):
        assert name in imported, f"{name} must be imported from Gaugefields and extended"
        assert name not in exported, f"{name} must not be exported as a function of its own"
    assert re.search(r"(?m)^Gradientflow\(U::Vector\{HIPLink\};", SRC)
    assert re.search(r"(?m)^function flow!\(U::Vector\{HIPLink\}, gf::HIPGradientflow\)", SRC)


def test_deepcopy_of_the_links_copies_the_device_field():
    m = re.search(r"(?ms)^function Base\.deepcopy_internal\(U::Vector\{HIPLink\}, stackdict::IdDict\)\n(.*?)^end", SRC)
    assert m, "deepcopy(::Vector{HIPLink}) must make a new device field"
    assert "similar(U)" in m.group(1) and "substitute_U!(V, U)" in m.group(1)
