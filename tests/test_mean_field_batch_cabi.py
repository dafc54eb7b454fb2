"""CPU-only checks of the batched mean-field entry (``qs_mean_field_batch`` / ``_workspace`` / ``_plan``): the
workspace formula the header documents, every refused argument (no GPU is touched: the checks run before any HIP
call), and the plan hook -- passes = ceil(ND / G), and a geometry that does not know ND."""

import ctypes

import pytest

F64, C128 = 0, 1
FORMS = {"fp64": (F64, F64, 2, 1), "complex128": (C128, C128, 1, 2), "mixed": (F64, C128, 2, 2)}
PLAN_FIELDS = ("G", "passes", "Rc", "nchunk", "ct_log", "ncb", "nrb", "lds_bytes", "grid")
SHIPPED_G = {"fp64": 8, "complex128": 4, "mixed": 4}


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from quantum_systems_amd import _lib

    return _lib.load()


def plan_of(lib, form, L, P, R, ND):
    u_dtype, d_dtype = FORMS[form][:2]
    out = (ctypes.c_int64 * 9)()
    assert lib.qs_mean_field_batch_plan(u_dtype, d_dtype, L, P, R, ND, ctypes.cast(out, ctypes.c_void_p), 9) == 0
    return dict(zip(PLAN_FIELDS, out))


def documented(form, L, R):
    """include/qs_amd.h: the tile geometry, G and Rc from (dtypes, L, R) alone."""
    _, _, cpi, aw = FORMS[form]
    Le, items = (L + 1) // 2 * 2, cdiv(L, cpi)
    best = None
    for lg in range(3, 8):
        ct, rb = 1 << lg, (256 >> lg) * 4
        area = cdiv(items, ct) * ct * cdiv(L, rb) * rb
        if best is None or area <= best[0]:
            best = (area, lg)
    lg = best[1]
    CT, RB = 1 << lg, (256 >> lg) * 4
    ncb, nrb = cdiv(items, CT), cdiv(L, RB)
    words = lambda rc, G: (rc * Le + nrb * RB + ncb * CT * cpi) * G * aw  # noqa: E731
    G = SHIPPED_G[form]
    while G > 1 and words(1, G) > 8192:
        G //= 2
    rc = cdiv(R, min(cdiv(4096, L), R))
    while rc > 1 and words(rc, G) > 8192:
        rc -= 1
    return dict(G=G, Rc=rc, nchunk=cdiv(R, rc), ct_log=lg, ncb=ncb, nrb=nrb, lds_bytes=8 * words(rc, G))


@pytest.mark.parametrize("form", list(FORMS))
def test_workspace_is_densities_times_rows_times_chunks(lib, form):
    u_dtype, d_dtype, _, aw = FORMS[form]
    es = 8 * aw
    for L, P, R in [(1, 1, 1), (5, 5, 5), (5, 2, 5), (31, 31, 7), (64, 64, 64), (96, 17, 96), (256, 256, 256),
                    (256, 32, 256), (256, 256, 32), (513, 2, 100), (1024, 3, 1024)]:
        doc = documented(form, L, R)
        for ND in (1, 2, 7, 8, 9, 33):
            got = lib.qs_mean_field_batch_workspace(u_dtype, d_dtype, L, P, R, ND)
            assert got == ND * P * L * doc["nchunk"] * es, (L, P, R, ND)
            assert got == P * lib.qs_mean_field_batch_workspace(u_dtype, d_dtype, L, 1, R, ND)       # linear in P
            assert got == ND * lib.qs_mean_field_batch_workspace(u_dtype, d_dtype, L, P, R, 1)       # and in ND
    q = lib.qs_mean_field_batch_workspace
    assert q(C128, F64, 8, 8, 8, 2) == -6 and q(7, F64, 8, 8, 8, 2) == -6
    assert q(u_dtype, d_dtype, 0, 1, 1, 2) == -1 and q(u_dtype, d_dtype, 8, 9, 8, 2) == -1
    assert q(u_dtype, d_dtype, 8, 8, 9, 2) == -1 and q(u_dtype, d_dtype, 8, 8, 0, 2) == -1
    assert q(u_dtype, d_dtype, 8, 8, 8, 0) == -1 and q(u_dtype, d_dtype, 8, 8, 8, -3) == -1
    assert q(u_dtype, d_dtype, 1025, 1, 1, 1) == -1


def test_refused_arguments_without_gpu(lib):
    # fake, well-separated device addresses: every call below returns before any HIP call is made
    u, D, W, work = 1 << 40, 2 << 40, 3 << 40, 4 << 40
    L, P, R, ND = 8, 8, 8, 3
    need = lib.qs_mean_field_batch_workspace(F64, F64, L, P, R, ND)
    weights = (ctypes.c_double * 8)(*([1.0] * 8))
    wp = ctypes.cast(weights, ctypes.c_void_p)

    def call(u_dtype=F64, d_dtype=F64, u=u, D=D, W=W, L=L, P=P, R=R, r_lo=0, ND=ND, cj=wp, ck=wp, work=work, nbytes=need):
        return lib.qs_mean_field_batch(u_dtype, d_dtype, u, D, W, L, P, R, r_lo, ND, cj, ck, work, nbytes, None)

    assert call(u=None) == -2 and call(D=None) == -2 and call(W=None) == -2 and call(work=None) == -2
    assert call(cj=None) == -2 and call(ck=None) == -2
    assert call(L=0) == -1 and call(L=-3) == -1
    assert call(P=0) == -1 and call(P=9) == -1 and call(R=0) == -1
    assert call(ND=0) == -1 and call(ND=-1) == -1
    assert call(R=4, r_lo=5) == -1 and call(R=4, r_lo=-1) == -1
    assert call(u_dtype=C128, d_dtype=F64) == -6
    assert call(u_dtype=3) == -6 and call(d_dtype=-1) == -6
    assert call(u_dtype=3, u=None) == -6 and call(L=0, u=None) == -1        # order: dtype pair, extents, null
    assert call(nbytes=need - 1) == -4
    assert call(u=u + 4) == -3 and call(D=D + 4) == -3 and call(W=W + 4) == -3 and call(work=work + 8) == -3
    assert call(u_dtype=C128, d_dtype=C128, u=u + 8, nbytes=2 * need) == -3
    assert call(W=u) == -7 and call(W=D) == -7 and call(W=work) == -7
    assert call(W=u + 8 * (P * R * L * L - 1)) == -7                          # W starts inside u
    assert call(W=D + 8 * (ND * L * L - 1)) == -7                             # ... inside the LAST density
    assert call(W=D - 8) == -7                                                # W reaches into D
    assert call(W=work, nbytes=0) == -7                                       # alias is reported before the size


def test_binding_and_wrapper(lib):
    import torch

    from quantum_systems_amd import _lib, kernels

    for name in ("qs_mean_field_batch", "qs_mean_field_batch_workspace", "qs_mean_field_batch_plan"):
        assert name in _lib.SIGNATURES
    assert lib.qs_abi_version() == 4
    with pytest.raises(RuntimeError, match="GPU only"):
        kernels.mean_field_batch(torch.zeros(3, 3, 3, 3, dtype=torch.float64), torch.zeros(2, 3, 3, dtype=torch.float64))


@pytest.mark.parametrize("form", list(FORMS))
def test_plan_does_not_know_the_batch(lib, form):
    u_dtype, d_dtype, cpi, aw = FORMS[form]
    for L in list(range(1, 131)) + [145, 204, 255, 256, 257, 322, 449, 512, 513, 895, 960, 1015, 1023, 1024]:
        for R in sorted({1, min(L, 2), L // 3 + 1, L}):
            doc = documented(form, L, R)
            G = doc["G"]
            seen = set()
            for ND in sorted({1, max(1, G - 1), G, G + 1, 3 * G}):
                for P in sorted({1, L}):
                    plan = plan_of(lib, form, L, P, R, ND)
                    where = (form, L, R, ND, P, plan)
                    assert plan["passes"] == cdiv(ND, plan["G"]), where
                    assert plan["grid"] == P * plan["nchunk"], where
                    assert all(plan[k] == doc[k] for k in doc), (where, doc)
                    assert plan["lds_bytes"] <= 65536, where
                    assert lib.qs_mean_field_batch_workspace(u_dtype, d_dtype, L, P, R, ND) == \
                        ND * P * L * plan["nchunk"] * 8 * aw, where
                    seen.add(tuple(plan[k] for k in ("G", "Rc", "nchunk", "ct_log", "ncb", "nrb", "lds_bytes")))
            assert len(seen) == 1, (form, L, R, seen)
    assert plan_of(lib, form, 128, 1, 128, 1)["G"] == SHIPPED_G[form]
    assert plan_of(lib, form, 256, 1, 256, 1)["G"] == SHIPPED_G[form]


def test_tuning_key_sets_the_group_size_and_resets(lib):
    from quantum_systems_amd import kernels

    L = 128
    for form, (u_dtype, d_dtype, _, aw) in FORMS.items():
        shipped = plan_of(lib, form, L, L, L, 5)
        assert shipped["G"] == SHIPPED_G[form]
        for G in (1, 2, 4, 8):
            with kernels.tuning(mean_field_batch_g=G):
                plan = plan_of(lib, form, L, L, L, 5)
                assert plan["G"] == G and plan["passes"] == cdiv(5, G), (form, G, plan)
                assert plan["lds_bytes"] <= 65536 and plan["Rc"] >= 1
                assert lib.qs_mean_field_batch_workspace(u_dtype, d_dtype, L, L, L, 5) == 5 * L * L * plan["nchunk"] * 8 * aw
            assert plan_of(lib, form, L, L, L, 5) == shipped, (form, G)       # the knob is gone after the block
        with kernels.tuning(mean_field_batch_g=0):                            # 0 = the shipped size
            assert plan_of(lib, form, L, L, L, 5) == shipped
    try:
        for bad in (-1, 3, 5, 6, 7, 9, 16):
            assert lib.qs_tuning_set(b"mean_field_batch_g", bad) == -1
            assert plan_of(lib, "fp64", L, L, L, 5)["G"] == SHIPPED_G["fp64"]  # a refused value changes nothing
        assert lib.qs_tuning_set(b"mean_field_batch_g", 2) == 0 and plan_of(lib, "fp64", L, L, L, 5)["G"] == 2
    finally:
        lib.qs_tuning_reset()
    assert plan_of(lib, "fp64", L, L, L, 5)["G"] == SHIPPED_G["fp64"]


def test_weights_are_a_scalar_or_one_per_density():
    import numpy as np
    import torch

    from quantum_systems_amd import kernels

    for scalar in (2, 2.0, np.float64(2.0), np.array(2.0), torch.tensor(2.0)):          # 0-d arrays are scalars
        assert list(kernels._weights(scalar, 3, "cj")) == [2.0, 2.0, 2.0]
    for seq in ([1.0, 0.0, -0.5], (1, 0, -0.5), np.array([1.0, 0.0, -0.5]), torch.tensor([1.0, 0.0, -0.5])):
        assert list(kernels._weights(seq, 3, "ck")) == [1.0, 0.0, -0.5]
    for seq in ([1.0], np.array([1.0, 2.0]), torch.ones(4), []):
        with pytest.raises(ValueError, match="ck has"):
            kernels._weights(seq, 3, "ck")


def test_plan_hook_refuses_what_the_workspace_query_refuses(lib):
    out = (ctypes.c_int64 * 10)(*([-99] * 10))
    ptr = ctypes.cast(out, ctypes.c_void_p)
    for args in [(C128, F64, 8, 8, 8, 2), (7, F64, 8, 8, 8, 2), (F64, -1, 8, 8, 8, 2), (F64, F64, 0, 1, 1, 2),
                 (F64, F64, 1025, 1, 1, 2), (F64, F64, 8, 9, 8, 2), (F64, F64, 8, 0, 8, 2), (F64, C128, 8, 8, 9, 2),
                 (C128, C128, 8, 8, 0, 2), (F64, F64, 8, 8, 8, 0), (C128, C128, 8, 8, 8, -1)]:
        refused = lib.qs_mean_field_batch_workspace(*args)
        assert refused < 0 and lib.qs_mean_field_batch_plan(*args, ptr, 9) == refused, args
    assert lib.qs_mean_field_batch_plan(F64, F64, 8, 8, 8, 2, ptr, 8) == -1      # short n_out
    assert lib.qs_mean_field_batch_plan(F64, F64, 8, 8, 8, 2, None, 9) == -2
    assert list(out) == [-99] * 10                                               # a refused call writes nothing
    assert lib.qs_mean_field_batch_plan(F64, F64, 8, 8, 8, 2, ptr, 10) == 0
    assert out[9] == -99 and all(x > 0 for x in out[:9])                         # nine values, no more
