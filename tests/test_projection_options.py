"""The projection's options record (projection.splat_options -> SplatOptions) and the names gs_model re-exports from the
modules its code moved to.  No GPU: nothing here touches the library."""
import pytest

from simplegaussiansplat_tk71_amd import density, gs_model, loss, optim, projection

# (centres, cov_dilation, clamp_colour, antialias) -> None, or (the record's fields, flags, mean_offset)
TABLE = [
    (("pixel", None, False, False), None),
    (("pixel", 1e-6, False, False), ((False, 1e-6, False, False), 0, 0.0)),
    (("subpixel", None, False, False), ((True, 1e-6, False, False), 0, 0.5)),
    (("pixel", None, True, False), ((False, 1e-6, True, False), 1, 0.0)),
    (("pixel", 0.3, False, True), ((False, 0.3, False, True), 2, 0.0)),
    (("subpixel", 0.3, True, True), ((True, 0.3, True, True), 3, 0.5)),
]


@pytest.mark.parametrize("options, want", TABLE, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) and len(v) == 4 else "")
def test_splat_options_table(options, want):
    got = projection.splat_options(*options)
    if want is None:
        assert got is None
        return
    fields, flags, mean_offset = want
    assert isinstance(got, projection.SplatOptions)
    assert got == fields and got._fields == ("subpixel", "cov_eps", "clamp_colour", "antialias")
    assert (got.subpixel, got.cov_eps, got.clamp_colour, got.antialias) == fields
    assert type(got.cov_eps) is float and type(got.subpixel) is bool and type(got.clamp_colour) is bool and type(got.antialias) is bool
    assert got.flags == flags and type(got.flags) is int
    assert got.mean_offset == mean_offset and type(got.mean_offset) is float


def test_antialias_defaults_to_false_and_an_integer_dilation_becomes_a_float():
    assert projection.splat_options("pixel", None, False) is None
    got = projection.splat_options("subpixel", 1, False)
    assert got == (True, 1.0, False, False) and type(got.cov_eps) is float


# gs_model.__all__ as it stood before the split, and where each name lives now (None: still gs_model's own)
EXPORTS = {
    "GS_dataset": None,
    "GS_model_with_param": None,
    "HipAdam": optim,
    "accumulate_screen_grads": density,
    "camera_inputs": projection,
    "qvec_to_rotmat_batch": None,
    "get_expon_lr_func": None,
    "mean_neighbour_distance": None,
    "splat_loss": loss,
}
PRIVATE = {"_box_clamp": projection, "SH_FRAMES": projection, "CENTRES": projection, "DENSIFY_ON": density}


def test_gs_model_exports_what_it_exported():
    assert set(EXPORTS) <= set(gs_model.__all__)
    for name, home in {**EXPORTS, **PRIVATE}.items():
        assert hasattr(gs_model, name), name
        if home is not None:
            assert getattr(gs_model, name) is getattr(home, name), name
        else:
            assert getattr(gs_model, name).__module__ == gs_model.__name__, name
    assert gs_model.SH_FRAMES == {"camera": 0, "world": 1}
    assert gs_model.CENTRES == ("pixel", "subpixel") and gs_model.DENSIFY_ON == ("position", "screen")
