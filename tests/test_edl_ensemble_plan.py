"""CPU side of the 1D ensembles (gmpnp_amd.edl_ensemble, gmpnp_amd.edl_sweep): the library exports the ensemble entry points,
members are planned and refused before anything touches a device, and member directories are named as EDLRun names them."""
import pytest

from gmpnp_amd import edl_ensemble as ee
from gmpnp_amd import edl_sweep
from gmpnp_amd.edl1d import run_identifier
from gmpnp_amd.params import edl_parameters

ENSEMBLE_SYMBOLS = ["gmpnp_ensemble_create", "gmpnp_ensemble_destroy", "gmpnp_ensemble_size", "gmpnp_ensemble_newton_solve",
                    "gmpnp_ensemble_member_error", "gmpnp_ensemble_assign_previous", "gmpnp_ensemble_get_state"]


def test_library_exports_the_ensemble_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from gmpnp_amd import backend
    lib = backend.load_library()
    for n in ENSEMBLE_SYMBOLS:
        assert n in backend.EXPORTS and hasattr(lib, n), n


def test_cartesian_product_order_and_size():
    m = ee.sweep_members([-2.5, -5.0, -7.5], ["K", "Cs"], [0.1, 0.5], model="PNP")
    assert len(m) == 12
    assert [(d["voltage_multiplier"], d["cation"], d["concentration_elec"]) for d in m[:5]] == [
        (-2.5, "K", 0.1), (-2.5, "K", 0.5), (-2.5, "Cs", 0.1), (-2.5, "Cs", 0.5), (-5.0, "K", 0.1)]
    assert all(d["model"] == "PNP" for d in m)
    args = edl_sweep.build_parser().parse_args(["--voltage_multiplier", "-2.5", "-5", "--cation", "K", "Cs", "--num_steps", "5"])
    assert args.voltage_multiplier == [-2.5, -5.0] and args.cation == ["K", "Cs"] and args.concentration_elec == [0.1]
    assert not args.staged and args.num_steps == 5


def test_members_that_may_differ_are_planned():
    members = [{"voltage_multiplier": -1.0}, {"voltage_multiplier": -5.0, "cation": "Cs"}, {"voltage_multiplier": -5.0, "concentration_elec": 0.5},
               {"voltage_multiplier": -10.0, "H_OHP": 1.0}, {"voltage_multiplier": -5.0, "model": "PNP"},
               {"voltage_multiplier": -5.0, "H2_FE": 0.5, "current_OHP_ss": 20.0}]
    kw, eps, steps = ee.plan_members(members, num_steps=100)
    assert len(kw) == 6 and steps == 100 and kw[1]["cation"] == "Cs" and kw[4]["model"] == "PNP"
    _, eps, steps = ee.plan_members([{"voltage_multiplier": -1.0}])
    assert steps == eps[0].tot_num_steps


@pytest.mark.parametrize("field,a,b", [("L_n", 50e-6, 1e-6), ("mesh_structure", "variable", "uniform"),
                                       ("dry_run", True, False), ("num_steps", 5, 6)])
def test_members_on_other_meshes_or_schedules_are_refused(field, a, b):
    with pytest.raises(ValueError, match=field):
        ee.plan_members([{"voltage_multiplier": -1.0, field: a}, {"voltage_multiplier": -5.0, field: b}])


def test_refused_configurations():
    with pytest.raises(ValueError, match="stabilization"):
        ee.plan_members([{"model": "PNP", "stabilization": "Y"}])
    with pytest.raises(ValueError):
        ee.plan_members([])
    with pytest.raises(ValueError):
        ee.plan_members([{"voltage_multiplier": -1.0}] * 65)
    with pytest.raises(TypeError):
        ee.plan_members([{"voltage": -1.0}])
    ee.plan_members([{"model": "MPNP", "stabilization": "Y"}])   # MPNP: the reference only warns


@pytest.mark.parametrize("kw", [{"voltage_multiplier": -5.0}, {"voltage_multiplier": -10.0, "cation": "Cs", "H_OHP": 1.0},
                                {"voltage_multiplier": -2.5, "model": "PNP", "H2_FE": 0.5, "current_OHP_ss": 20.0}])
def test_member_directory_is_the_serial_identifier(kw):
    full = dict(ee.MEMBER_DEFAULTS, **kw)
    assert ee.member_identifier(kw) == run_identifier(edl_parameters(**full), full)
    if kw == {"voltage_multiplier": -5.0}:
        assert ee.member_identifier(kw) == "voltage_-5.0_H2_FE_0.2_current_10.0_H_OHP_None_cation_K"


def test_error_text_is_the_serial_drivers():
    from gmpnp_amd import backend
    assert ee.error_text(backend.ERR_NOT_CONVERGED, "x") == "Newton solver did not converge because maximum number of iterations reached"
    assert ee.error_text(backend.ERR_NUMERIC, "residual became NaN") == str(backend.GmpnpError(backend.ERR_NUMERIC, "residual became NaN"))
