"""Every case of tests/instantiation_cases.py on the MI355X: the case's own check on the shipped kernels.  Which instantiation a case
reaches is asserted by the host-emulated twin, tests/test_emu_instantiations.py; it transfers because dispatch depends on the
arguments, on alignment and on the CU count only, and the fixture below refuses a device whose CU count is not the emulation's."""
import pytest

from tests import instantiation_cases as ic
from tests import rate_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    import torch
    assert torch.cuda.is_available()
    b = ic.gpu_backends()
    assert b.cus == ic.CUS, ("this device has %d compute units, the emulated build answers %d: the form switches sit elsewhere and the "
                             "instantiations claimed in tests/instantiation_cases.py need not be the ones that run here" % (b.cus, ic.CUS))
    return b


@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.id)
def test_instantiation(bk, case):
    case.run(bk)


@pytest.mark.parametrize("F", rc.NH3_FS)
def test_spectral_peak_either_side_of_the_form_switch_at_three_frequency_tiles(bk, F):
    rc.check_form_switch(bk.rate, T=16, F=F)
