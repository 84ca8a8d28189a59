"""run_input.average_fields in the host mirror (src/input.cpp:115-133): the names are stored lower-cased, a name outside
the reference's five and w_average in a two-dimensional case are refused, and a case has none by default.  Host only."""
import pytest

import hfx
import hfx_host as H

NAMES = ["rho_average", "u_average", "v_average", "w_average", "e_average"]


@pytest.fixture()
def case3():
    c = H.Case(3, order=1)
    yield c
    c.close()


@pytest.fixture()
def case2():
    c = H.Case([3, 3, 1], dims=2, order=1)
    yield c
    c.close()


def test_no_average_fields_by_default(case3):
    assert case3.average_fields() == []
    assert case3.clock()[1] == 0


def test_names_are_lower_cased(case3):
    case3.set_average_fields(["Rho_Average", "U_AVERAGE", "v_average", "W_average", "E_Average"])
    assert case3.average_fields() == NAMES
    # the order of the input file is kept, and a name may repeat
    case3.set_average_fields(["e_average", "RHO_average", "e_average"])
    assert case3.average_fields() == ["e_average", "rho_average", "e_average"]
    case3.set_average_fields([])
    assert case3.average_fields() == []


@pytest.mark.parametrize("bad", ["p_average", "rho", "", "u_average "])
def test_unknown_name_is_refused(case3, bad):
    case3.set_average_fields(["u_average"])
    with pytest.raises(hfx.HfxError, match="unknown"):
        case3.set_average_fields(["rho_average", bad])
    assert case3.average_fields() == ["u_average"]  # a refusal leaves the case as it was


def test_w_average_is_refused_in_2d(case2):
    with pytest.raises(hfx.HfxError, match="w_average"):
        case2.set_average_fields(["u_average", "W_average"])
    assert case2.average_fields() == []
    case2.set_average_fields(["rho_average", "u_average", "v_average", "e_average"])
    assert case2.average_fields() == ["rho_average", "u_average", "v_average", "e_average"]
