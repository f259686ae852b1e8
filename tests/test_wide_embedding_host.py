"""Host-side queries of the loss at `embedding_dim` 64 .. 256 (no device needed): `iisan_inbatch_ce_route_e` and
`iisan_inbatch_ce_ws_bytes_e` against the 64-wide queries they generalise, under every `ce_fast`."""
import pytest

from iisan_amd import _lib

SHAPES = [(7, 5), (37, 10), (6, 15), (9, 3), (4, 16), (1024, 10), (2048, 10)]


@pytest.mark.parametrize("bs,S", SHAPES)
def test_route_and_workspace_queries_by_width(lib, bs, S):
    """At 64 the two are the queries without a width.  At 128 / 192 / 256 the route is the 64-wide one except that the split-operand
    route (3: `ce_fast` 3, or `ce_fast` 1 from 2^24 logits on) becomes the fused f32 route (2); the workspace holds no operand images
    and grows by the d_prec buffer's 4 bs S 64 bytes per 64 features.  Widths outside the set: -1 and 0 bytes."""
    sizes = {}
    for E in (64, 128, 192, 256):
        for ce_fast in (1, 0, 2, 3, 4):
            with _lib.dev(ce_fast=ce_fast):
                r64, r = lib.iisan_inbatch_ce_route(bs, S), lib.iisan_inbatch_ce_route_e(bs, S, E)
            assert r == (r64 if E == 64 or r64 != 3 else 2), (E, ce_fast, r64, r)
        sizes[E] = lib.iisan_inbatch_ce_ws_bytes_e(bs, S, E)
    assert sizes[64] == lib.iisan_inbatch_ce_ws_bytes(bs, S) > 0
    assert sizes[128] < sizes[64]
    pad = 256                                    # (each carve of the workspace is aligned: the difference is 16,384 bs S up to one alignment)
    for lo, hi in ((128, 192), (192, 256)):
        assert 0 <= sizes[hi] - sizes[lo] - 4 * bs * S * 64 <= pad, (lo, hi, sizes)
    for E in (0, 32, 96, 320, -64):
        assert lib.iisan_inbatch_ce_route_e(bs, S, E) == -1 and lib.iisan_inbatch_ce_ws_bytes_e(bs, S, E) == 0


def test_queries_refuse_windows_outside_one_to_sixty_three(lib):
    for S in (0, 64):
        assert lib.iisan_inbatch_ce_route_e(3, S, 128) == -1 and lib.iisan_inbatch_ce_ws_bytes_e(3, S, 128) == 0
    assert lib.iisan_inbatch_ce_route_e(0, 10, 128) == -1 and lib.iisan_inbatch_ce_ws_bytes_e(0, 10, 128) == 0
