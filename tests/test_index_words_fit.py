"""CPU: the fit rule of the index words the resident iterate keeps in registers (host_core.hpp index_words_fit, DESIGN.md
section 3 "Index words in registers").  A thread of a tile walks entries e = tid + j * threads of xloc in the D^-1 pass
((n + m) * tile entries) and of pinv in the two loops of the vector step (n * tile and m * tile entries); the words stay in
registers where the handle keeps the resident state with the solve vector in LDS and no thread has more trips than the
caps: xloc_trips through xloc, pinv_trips through either kind of row."""
import pytest

import osqp_solver_amd as M


def _fit(n, m, **kw):
    return M.debug_index_words_fit(n, m, **kw)[0]


def test_caps_hold_the_headline_shape_in_two_registers():
    fit, xt, pt = M.debug_index_words_fit(512, 1024)
    assert fit and xt >= 2 and pt >= 1            # config 3 at 1024 threads: N = 2 * threads, n < threads, m = threads
    assert (xt + 1) // 2 + pt <= 4                # 16-bit positions, two to a register


@pytest.mark.parametrize("threads", [1024, 640])
@pytest.mark.parametrize("tile", [1, 2])
def test_boundaries_of_the_three_counts(threads, tile):
    _, xt, pt = M.debug_index_words_fit(1, 0, tile=tile, threads=threads)
    cap_p, cap_x = pt * threads // tile, xt * threads // tile       # rows of one kind / rows in all a tile's threads cover
    kw = dict(tile=tile, threads=threads)
    # the x rows alone
    assert _fit(cap_p, 0, **kw) and not _fit(cap_p + 1, 0, **kw)
    # the z / y rows, beside one x row
    assert _fit(1, min(cap_p, cap_x - 1), **kw) and not _fit(1, cap_p + 1, **kw)
    # the rows of the D^-1 pass: at the committed caps (xloc 2, pinv 1) cap_x == 2 cap_p, so the rule's third condition,
    # (n + m) tile <= cap_x threads, follows from the other two and has no boundary of its own to test; its corner is
    # both kinds of row at their cap at once
    assert cap_x == 2 * cap_p
    assert _fit(cap_p, cap_p, **kw) and not _fit(cap_p + 1, cap_p, **kw) and not _fit(cap_p, cap_p + 1, **kw)
    assert _fit(1, 0, **kw) and _fit(1, 1, **kw)


def test_needs_the_resident_state_and_the_lds_vector():
    assert _fit(96, 160)
    assert not _fit(96, 160, resident_state=False)
    assert not _fit(96, 160, lds_vector=False)
    assert not _fit(96, 160, resident_state=False, lds_vector=False)


def test_a_resident_shape_over_the_cap():
    """n = m = 1100 at 1024 threads: state and vector fit LDS, but n and m need two trips each and N three."""
    _, xt, pt = M.debug_index_words_fit(1, 0)
    assert (xt, pt) == (2, 1)
    assert not _fit(1100, 1100) and not _fit(1100, 100) and not _fit(100, 1100) and _fit(1024, 1024)


def test_invalid_arguments_are_refused():
    for kw in (dict(n=0, m=1), dict(n=1, m=-1), dict(n=1, m=1, tile=3), dict(n=1, m=1, threads=0), dict(n=1, m=1, threads=96),
               dict(n=1, m=1, threads=2048), dict(n=2 ** 30, m=1)):
        with pytest.raises(M.MiOsqpError) as e:
            M.debug_index_words_fit(**kw)
        assert e.value.code == 1
