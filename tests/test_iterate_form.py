"""CPU: the form of the resident head of S^-1 an iterate launch takes (host_core.hpp iterate_form, DESIGN.md section 3
"Resident head of S^-1"): 0 the streaming form (a handle without a head), 1 the deep ring, 2 the long head.  A launch that
iterates at least `long_min` tiles (MI_OSQP_RF_LONG_MIN) takes the long head, a smaller one the deep ring; the default is 0 -
every launch that iterates anything takes the long head.  MI_OSQP_RF_FORM forces one form for every launch of a handle that
has a head."""
import pytest

import osqp_solver_amd as M

STREAMED, DEEP, LONG = 0, 1, 2


def test_by_default_every_launch_with_a_tile_takes_the_long_head():
    for tiles in (1, 2, 31, 201, 1024, 2 ** 31 - 1):
        assert M.debug_iterate_form(tiles) == LONG
        assert M.debug_iterate_form(tiles, long_min=-1) == M.debug_iterate_form(tiles, long_min=0) == LONG


@pytest.mark.parametrize("long_min", [1, 2, 5, 32, 128, 1024, 2 ** 31 - 1])
def test_explicit_threshold_edges(long_min):
    if long_min > 1:
        assert M.debug_iterate_form(long_min - 1, long_min=long_min) == DEEP
        assert M.debug_iterate_form(1, long_min=long_min) == DEEP
    assert M.debug_iterate_form(long_min, long_min=long_min) == LONG
    if long_min < 2 ** 31 - 1:
        assert M.debug_iterate_form(long_min + 1, long_min=long_min) == LONG
    assert M.debug_iterate_form(2 ** 31 - 1, long_min=long_min) == LONG


def test_zero_tiles_take_the_deep_ring_at_every_threshold():
    """A launch that iterates nothing does nothing in either form; it is not counted as a launch of the long head."""
    for long_min in (-1, 0, 1, 128):
        assert M.debug_iterate_form(0, long_min=long_min) == DEEP


def test_a_handle_without_a_head_streams_whatever_is_asked():
    for tiles in (0, 1, 128, 1024):
        for forced in (0, DEEP, LONG):
            for long_min in (-1, 0, 128):
                assert M.debug_iterate_form(tiles, has_head=False, forced_form=forced, long_min=long_min) == STREAMED


def test_forced_forms_ignore_the_threshold():
    for tiles in (0, 1, 127, 128, 1024):
        for long_min in (-1, 0, 128, 2 ** 31 - 1):
            assert M.debug_iterate_form(tiles, forced_form=DEEP, long_min=long_min) == DEEP
            assert M.debug_iterate_form(tiles, forced_form=LONG, long_min=long_min) == LONG


def test_invalid_arguments_are_refused():
    for kw in (dict(tiles=-1), dict(tiles=2 ** 31), dict(tiles=1, forced_form=3), dict(tiles=1, forced_form=-1), dict(tiles=1, long_min=-2),
               dict(tiles=1, long_min=2 ** 31)):
        with pytest.raises(M.MiOsqpError) as e:
            M.debug_iterate_form(**kw)
        assert e.value.code == 1
