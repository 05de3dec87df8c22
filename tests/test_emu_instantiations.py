"""Every case of tests/instantiation_cases.py on the host-emulated build (tests/emu): the case's own check, and the launch census'
word that the instantiation the case claims is the one that ran (tests/emu/include/hip/hip_runtime.h, DESIGN.md "Launch census").
The GPU twin, without the reach assertion, is tests/test_gpu_instantiations.py."""
import pytest

from tests import emu_harness
from tests import instantiation_cases as ic


@pytest.fixture(scope="module")
def bk():
    return ic.emu_backends(emu_harness.Emu())


def test_references_alone_meet_their_caps_on_the_new_inputs():
    ic.check_references_alone()


def test_every_claim_is_an_instantiation_of_the_emulated_library(bk):
    universe = emu_harness.census_universe(bk.lib)
    assert len(universe) > 500
    missing = sorted({n for c in ic.CASES for n in c.claims} - universe)
    assert not missing, missing


def test_the_census_marks_what_is_launched_and_nothing_else(bk):
    emu_harness.census_reset(bk.lib)
    assert emu_harness.census_launched(bk.lib) == frozenset()
    ic.puc.check_block_sums(bk.pulse, 3, 5, 4, 1)
    assert emu_harness.census_launched(bk.lib) == {"rm::k_bgr_block_sums<4, false>"}
    emu_harness.census_reset(bk.lib)
    assert emu_harness.census_launched(bk.lib) == frozenset()


@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.id)
def test_emu_instantiation(bk, case):
    emu_harness.census_reset(bk.lib)
    case.run(bk)
    launched = emu_harness.census_launched(bk.lib)
    missing = [n for n in case.claims if n not in launched]
    assert not missing, (case.id, case.entry, "claimed but not launched", missing, sorted(launched))
