"""tests/pipeline_matrix.py held to what it claims: every committed row is valid, every pair of factor values that some valid row can hold
is in a row, the caps hold, the tables are the generator's, and ``refusal`` restates the product -- the pipelines' device-free checks
(``_check_sigma``, ``_pixel_format``, ``_Finish``, ``_check_cuts_mode``, the format's ``geometry``) raise exactly where it says so."""
import inspect
import itertools
import types

import numpy as np
import pytest

import pipeline_matrix as M

PIPELINES = M.PIPELINES
ROWS = M.ROWS


def _key(a, b):
    return tuple(sorted([a, b], key=lambda kv: kv[0]))


def _first_full_row(fixed, fac, accept):
    """the first full row over ``fac`` that holds ``fixed`` and that ``accept`` takes, from the plain product; None if there is none"""
    rest = [n for n in fac if n not in fixed]
    for vals in itertools.product(*(fac[n] for n in rest)):
        row = dict(fixed, **dict(zip(rest, vals)))
        if accept(row):
            return row
    return None


def _brute_force_pairs(pipeline):
    """from the factor table and ``valid`` on full rows alone: the pairs some valid full row holds"""
    fac = M.factors(pipeline)
    items = [(n, v) for n, vs in fac.items() for v in vs]
    found = set()
    for a, b in itertools.combinations(items, 2):
        if a[0] == b[0] or _key(a, b) in found:
            continue
        row = _first_full_row(dict([a, b]), fac, lambda r: M.valid(r, pipeline))
        if row is not None:
            found |= M.pairs_of(row)                       # a valid row vouches for all of its pairs
    return found


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_every_row_is_valid_and_the_cap_holds(pipeline):
    rows = ROWS[pipeline]
    assert 0 < len(rows) <= M.CAPS[pipeline]
    assert len(set(rows)) == len(rows)
    fac = M.factors(pipeline)
    for r in rows:
        d = M.as_dict(r, pipeline)
        assert all(d[n] in fac[n] for n in fac), r
        assert M.valid(d, pipeline), (r, M.refusal(d, pipeline), M.vacuous(d, pipeline))
    assert tuple(rows[:len(M.MANDATORY[pipeline])]) == tuple(M.MANDATORY[pipeline])


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_every_jointly_valid_pair_is_in_a_row(pipeline):
    want = _brute_force_pairs(pipeline)
    have = set()
    for r in ROWS[pipeline]:
        have |= M.pairs_of(M.as_dict(r, pipeline))
    assert want - have == set(), sorted(want - have, key=repr)[:10]
    assert have <= want
    assert want == M.valid_pairs(pipeline)                 # the generator's own search agrees with the brute force
    fac = M.factors(pipeline)
    assert len(want) > 0.9 * sum(len(a) * len(b) for a, b in itertools.combinations(fac.values(), 2))       # the rules cut little


def test_the_two_formats_left_to_the_clip_table_are_there():
    assert {"rgb0", "x2rgb10le"} <= {r[0] for r in M.CLIP_ROWS} and not {"rgb0", "x2rgb10le"} & {r[0] for r in M.LIVE_ROWS}
    assert set(M.LIVE_PIX_FMT) | {"rgb0", "x2rgb10le"} == set(M.PIX_FMT)
    assert {r[0] for r in M.CLIP_ROWS} | {r[0] for r in M.CLIP2_ROWS} == set(M.PIX_FMT)            # every format meets ClipPipeline
    assert {r[2] for r in M.CLIP2_ROWS} == set(M.CLIP2_SIGMAS) and {r[2] for r in M.CLIP_ROWS} == set(M.SIGMAS)


def test_the_picture_without_a_detector_block_meets_auto_cuts_in_every_table():
    """6 x 10 with cuts='auto' is a pair the constructors take: LiveStream rows at depth 2 and more and rows of both ClipPipeline tables
    hold it (the GPU rows assert no cut and every score 0.0 there); every other cuts='auto' row must find a cut"""
    for pipeline in PIPELINES:
        hold = [M.as_dict(r, pipeline) for r in ROWS[pipeline] if r[1] == "6x10r" and r[3] == "auto"]
        assert hold and not any(M.finds_cuts(d) for d in hold)
        assert any(d["depth"] >= 2 for d in hold)
        assert all(M.finds_cuts(M.as_dict(r, pipeline)) for r in ROWS[pipeline] if r[3] == "auto" and r[1] != "6x10r")


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_the_committed_table_is_the_generator_s(pipeline):
    assert tuple(M.generate(pipeline)) == tuple(ROWS[pipeline])


# ---- refusal against the product -----------------------------------------------------------------------------------------------------------
def _stub(in_ch):
    return types.SimpleNamespace(net=types.SimpleNamespace(net_in_ch=in_ch))


def _product_refuses(row, pipeline, in_ch=4):
    """the pipelines' device-free checks in the constructors' order, then ``geometry`` on a zero frame (stream C: on one of the other
    size as well); the one option a pipeline has no argument for is read from its signature"""
    from bsvd_amd import pipeline as P
    what = "LiveStream" if pipeline == "live" else "ClipPipeline"
    if row["cuts"] == "manual" and pipeline != "live":
        return "cut" not in inspect.signature(P.ClipPipeline.submit).parameters
    kw = M.constructor_kw(row, pipeline)
    try:
        P._check_cuts_mode(kw["cuts"], P.CUT_THRESHOLD, what)
        P._check_sigma(_stub(in_ch), kw["sigma"], kw["sigma_gain"], what)
        fmt = P._pixel_format(kw["pix_fmt"], kw["colour"], kw["pad"], kw["frame_shape"])
        P._Finish(fmt, kw["strength"], kw["dither"], kw["dither_seed"], None)
        sizes = [M.size_of(row)[0]] + ([M.other_size(row)] if pipeline == "live" and row["stream"] == "C" else [])
        for size in sizes:
            shape, dtype = M.array_spec(row, pipeline, size)
            n = (3,) if pipeline == "clip" else ()
            fmt.geometry(np.zeros(n + shape, dtype), clip=pipeline == "clip")
    except ValueError:
        return True
    return False


@pytest.mark.parametrize("pipeline", ("live", "clip"))
def test_refusal_agrees_with_the_product_on_a_row_for_every_pair(pipeline):
    """every pair of values of the whole factor table (all eleven formats): one full row that holds it -- one the rules take if there is
    one, else the first of the product -- through the product's checks; they raise exactly where ``refusal`` speaks"""
    names = M.LIVE_FACTORS if pipeline == "live" else M.CLIP_FACTORS
    fac = {n: M.FACTORS[n] for n in names}
    items = [(n, v) for n, vs in fac.items() for v in vs]
    seen, refused, taken = set(), 0, 0
    for a, b in itertools.combinations(items, 2):
        if a[0] == b[0]:
            continue
        fixed = dict([a, b])
        row = None if M.refusal(fixed, pipeline) else _first_full_row(fixed, fac, lambda r: M.refusal(r, pipeline) is None)
        if row is None:
            row = _first_full_row(fixed, fac, lambda r: True)
        key = tuple(row[n] for n in names)
        if key in seen:
            continue
        seen.add(key)
        says = M.refusal(row, pipeline)
        assert _product_refuses(row, pipeline) == (says is not None), (row, says)
        refused, taken = refused + (says is not None), taken + (says is None)
    assert refused >= 10 and taken >= 100, (refused, taken)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_every_committed_row_passes_the_product_s_checks_and_a_blind_model_is_refused_where_sigma_needs_a_plane(pipeline):
    for r in ROWS[pipeline]:
        d = M.as_dict(r, pipeline)
        assert not _product_refuses(d, pipeline), r
        assert _product_refuses(d, pipeline, in_ch=3) == (d["sigma"] != "const"), r


def test_what_the_matrix_leaves_out_is_taken_by_the_product():
    """the ``vacuous`` rules are the matrix's own: the product takes those rows"""
    fac = {n: M.FACTORS[n] for n in M.LIVE_FACTORS}
    n = 0
    for fixed in (dict(pix_fmt="yuv420p", colour="rgb-limited"), dict(pix_fmt="p010", colour="rgb-limited")):
        row = _first_full_row(fixed, fac, lambda r: M.refusal(r, "live") is None)
        assert M.vacuous(row, "live") and not M.valid(row, "live") and not _product_refuses(row, "live")
        n += 1
    assert n == 2


def test_the_frames_of_every_format_and_size_are_what_the_format_s_geometry_takes():
    """tests/pipeline_by_hand.frames: shape and dtype of ``array_spec``, read-only, both ends of the code range, taken by ``geometry``"""
    import pipeline_by_hand as BH
    from bsvd_amd import pipeline as P
    for fmt in M.PIX_FMT:
        for size in M.SIZES:
            for pipeline, shape_key in (("live", "given"), ("live", "none"), ("clip", None)):
                row = dict(pix_fmt=fmt, size=size, colour="default", frame_shape=shape_key)
                if M.refusal(row, pipeline):
                    continue
                hw, pad = M.size_of(row)
                fr = BH.frames(fmt, hw, 3, seed=1, dark_from=2, one_d=M.one_d(row, pipeline))
                shape, dtype = M.array_spec(row, pipeline)
                assert fr.shape == (3,) + shape and fr.dtype == np.dtype(dtype) and not fr.flags.writeable
                f = P._pixel_format(fmt, M.colour_of(row), pad, hw if shape_key == "given" or fmt in M.YUV_1D else None)
                g = f.geometry(fr[0] if pipeline == "live" else fr, clip=pipeline == "clip")
                assert (g.h, g.w) == hw
                assert np.array_equal(fr, BH.frames(fmt, hw, 3, seed=1, dark_from=2, one_d=M.one_d(row, pipeline)))
                if fmt in M.ALPHA:
                    a = BH.alpha_of(fmt, fr, hw)
                    assert a.min() == 0 and a.max() == (1 << BH.BITS[fmt]) - 1
