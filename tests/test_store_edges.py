"""The premises of tests/test_gpu_store_edges.py without a GPU: every input recipe of tests/store_edges.py against its conditions, on the models
alone.  The conditions are statements about a MODEL's output -- its stores reach the binary16 subnormal range, the overflow boundary and -0
(shares counted over the cells the stage stores), or its fields are fp32 subnormals -- so that the bit-for-bit comparison of the GPU test is a
comparison there.  If a recipe misses one, the recipe is wrong, not the bound; each test prints the shares it reached.  The last tests hold the
lab switch WIDE_OFFSETS to its place: the lab build's, by name; the shipped library refuses it."""
import numpy as np
import pytest

import store_edges as se
from store_edges import ids

ADDRESSES = ["clamp", "mirror"]


@pytest.fixture(autouse=True)
def quiet_casts():
    with np.errstate(over="ignore"):                         # the models round past 65504 to inf on purpose
        yield


# ---- part 1: binary16 edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps,overflow", se.VORTICITY_HALF)
@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_vorticity_recipe(dims, eps, overflow):
    se.assert_conditions(se.vorticity_half(dims, eps))


@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_emitter_recipe_is_exact_and_reaches_the_edges(dims):
    """the two balls of store_edges.emitters_exact: no cell near the threshold, and a basis perturbed by 3e-7 relative (more than an ulp of exp2
    either way) leaves every output bit and the support mask unchanged -- so device and model, which evaluate exp2 differently, must agree
    bit for bit inside the supports too"""
    c = se.emit_half(dims)
    se.assert_conditions(c)
    assert se.perturbed_basis_changes_nothing(dims)
    assert not (np.signbit(c.col) & (c.col == 0)).any()      # no -0 among the colour inputs: saturate(-0) is a maximum of -0 and +0, which nobody fixes
    assert (c.want_col[c.touched] == 1).any() and (c.want_col[c.touched] == 0).any()


@pytest.mark.parametrize("address", ADDRESSES)
@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_heat_recipe(dims, address):
    se.assert_conditions(se.heat_half(dims, address))


@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_inflow_recipe(dims):
    c = se.inflow_half(dims)
    se.assert_conditions(c)
    assert (c.w == 0).any() and ((c.w > 0) & (c.w < 1)).any() and (c.w == 1).any()      # traces that leave by more than a cell, by less, not at all


@pytest.mark.parametrize("dims", se.BND_SHAPES, ids=ids)
def test_enforce_recipe(dims):
    se.assert_conditions(se.enforce_half(dims))


@pytest.mark.parametrize("name", se.PROJECT_SETTINGS)
@pytest.mark.parametrize("dims", se.BND_SHAPES, ids=ids)
def test_projection_recipe(dims, name):
    c = se.project_half(dims, name)
    se.assert_conditions(c)
    if name == "obstacles":                                  # the numpy model with no face open is the C++ obstacle reference, here too
        assert se.same_bits(c.want, se.ob.ref_project(c.vel, c.p, c.mask, True))


@pytest.mark.parametrize("address", ADDRESSES)
@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_maccormack_recipe(dims, address):
    se.assert_conditions(se.maccormack_half(dims, address))


# ---- part 2: fp32 subnormals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["log", "all"])
@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_vorticity_subnormal_recipe(dims, kind):
    c = se.vorticity_subnormal(dims, kind)
    se.assert_conditions(c)
    if kind == "all":
        assert se.same_bits(c.want, c.vel) and c.vel.any()   # the model returns the field bit for bit; a kernel that flushed would return zeros


@pytest.mark.parametrize("name", se.PROJECT_SETTINGS)
@pytest.mark.parametrize("dims", se.BND_SHAPES, ids=ids)
def test_pressure_subnormal_recipe(dims, name):
    c = se.pressure_subnormal(dims, name)
    se.assert_conditions(c)
    if name == "obstacles":
        assert se.same_bits(c.q, se.ob.ref_jacobi(c.p, c.b, c.mask, se.SWEEPS)) and se.same_bits(c.w, se.ob.ref_project(se.ob.ref_enforce(c.vel, np.zeros(c.p.shape + (4,), np.float32), c.mask)[0], c.q, c.mask))


@pytest.mark.parametrize("dims", se.MG_SHAPES, ids=ids)
def test_multigrid_subnormal_recipe(dims):
    se.assert_conditions(se.multigrid_subnormal(dims))
    levels = se.mg.plan(dims)
    assert len(levels) == {(36, 36, 1): 3, (64, 64, 4): 2, (70, 70, 4): 2, (20, 20, 8): 3, (70, 70, 5): 1}[dims]
    assert (se.mg.tail_level(levels) > 0) == (len(levels) > 1)         # every level below the first is small enough for k_mg_tail


@pytest.mark.parametrize("which", se.FIELD_INPUTS)
@pytest.mark.parametrize("dims", se.TILE_SHAPES, ids=ids)
def test_field_subnormal_recipe(dims, which):
    se.assert_conditions(se.field_subnormal(dims, which))


# ---- part 3: the lab switch -----------------------------------------------------------------------------------------------------------------
def test_the_shipped_library_does_not_know_wide_offsets():
    from fluidx12_amd import build, capi
    assert "WIDE_OFFSETS" in capi.LAB_KNOBS
    if build.LAB:
        return
    assert "WIDE_OFFSETS" not in capi.knob_names()
    assert capi.load().fx_set_knob(b"WIDE_OFFSETS", b"1") == capi.FX_E_INVALID
    assert capi.load().fx_set_knob(b"WIDE_OFFSETS", None) == capi.FX_E_INVALID


def test_the_lab_build_offers_the_shipped_switches_and_the_lab_ones():
    """capi.LAB_KNOBS is the list of fx_knobs.cpp under FX_LAB, name for name"""
    import conftest
    from fluidx12_amd import build, capi
    if build.LAB:                                            # (FLUIDX_BUILD_LAB=1: the library in the package is a lab build itself)
        return
    lab = conftest.lab_library()
    names, i = [], 0
    while lab.fx_knob_name(i) is not None:
        names.append(lab.fx_knob_name(i).decode())
        i += 1
    assert len(names) == len(set(names))
    assert set(names) == set(capi.knob_names()) | capi.LAB_KNOBS and not set(capi.knob_names()) & capi.LAB_KNOBS
    assert "WIDE_OFFSETS" in names
