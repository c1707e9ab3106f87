"""KID on the device, the parts that need no GPU: the estimator from the kernel's 6m+3 sums, the subset draw and its
effect on numpy's global generator, the argument checks of the C entry point, the runner key."""
import ctypes

import numpy as np
import pytest

from kid_support import activations, host_rows as _host_rows, numpy_sums


def test_estimator_from_sums_equals_the_matrix_form():
    from lightning_gan_zoo_amd import eval as E
    real, fake = activations(1, 400, 48, 0.0), activations(2, 360, 48, 0.3)
    np.random.seed(123)
    rows = _host_rows(400, 360, 7, 150)
    np.random.seed(123)
    mmds, variances = E.polynomial_mmd_averages(real, fake, n_subsets=7, subset_size=150)
    sums = np.stack([numpy_sums(real[a], fake[b]) for a, b in rows])
    assert sums.shape == (7, 6 * 150 + 3)
    got_m, got_v = E._mmd2_and_variance_from_sums(sums, 150, var_at_m=360, ret_var=True)
    assert np.allclose(got_m, mmds, rtol=1e-10, atol=0)
    assert np.allclose(got_v, variances, rtol=1e-8, atol=0)
    only = E._mmd2_and_variance_from_sums(sums, 150, var_at_m=360, ret_var=False)
    assert np.array_equal(only, got_m)
    # var_at_m defaults to m, as in the matrix form
    one = E.polynomial_mmd(real[rows[0][0]], fake[rows[0][1]])
    dflt = E._mmd2_and_variance_from_sums(sums[:1], 150)
    assert np.allclose([dflt[0][0], dflt[1][0]], one, rtol=1e-8, atol=0)
    with pytest.raises(ValueError):
        E._mmd2_and_variance_from_sums(sums[:, :-1], 150)


@pytest.mark.parametrize("n_g,n_r,n_subsets,subset_size", [(400, 360, 7, 150), (40, 30, 3, 1000), (5, 9, 2, 5)])
def test_draw_kid_subsets_is_the_host_loops_draw(n_g, n_r, n_subsets, subset_size):
    from lightning_gan_zoo_amd import eval as E
    g, r = np.arange(n_g, dtype=np.float64)[:, None] * np.ones(3), -np.arange(n_r, dtype=np.float64)[:, None] * np.ones(3)
    np.random.seed(77)
    rows = _host_rows(n_g, n_r, n_subsets, subset_size)
    np.random.seed(77)
    E.polynomial_mmd_averages(g, r, n_subsets=n_subsets, subset_size=subset_size)
    want = np.random.get_state()
    np.random.seed(77)
    idx = E.draw_kid_subsets(n_g, n_r, n_subsets, subset_size)
    have = np.random.get_state()
    assert idx.dtype == np.int32 and idx.shape == (n_subsets, 2, min(n_g, n_r, subset_size))
    assert np.array_equal(idx, rows)
    assert have[0] == want[0] and np.array_equal(have[1], want[1]) and have[2:] == want[2:]


def test_c_entry_point_checks_its_arguments_without_a_device():
    from lightning_gan_zoo_amd._lib import lib
    assert lib.gz_kid_workspace_bytes(100, 1000, 2048) % 8 == 0
    assert lib.gz_kid_workspace_bytes(1, 1, 1) <= lib.gz_kid_workspace_bytes(100, 1000, 2048) < (1 << 20)
    p = ctypes.c_void_p(0x1000)             # never dereferenced: every call below is refused before a launch

    def call(n_g=10, n_r=12, d=4, S=2, m=5, degree=3, g=p, r=p, idx=p, out=p, ws=p):
        return lib.gz_kid_sums(g, n_g, r, n_r, d, idx, S, m, 0.25, 1.0, degree, out, ws, 1 << 20, None)

    for bad in (dict(S=0), dict(m=0), dict(d=0), dict(degree=0), dict(n_g=0), dict(n_r=0), dict(S=-1), dict(m=-3),
                dict(m=11), dict(m=13), dict(n_g=4), dict(g=None), dict(r=None), dict(idx=None), dict(out=None),
                dict(ws=None)):
        assert call(**bad) == -1, bad


def test_runner_key_parses_and_defaults_to_false():
    from lightning_gan_zoo_amd.run_network import RUNNER_KEYS, parse_overrides
    assert RUNNER_KEYS["kid_on_device"] is False
    for plus in ("", "+"):
        run = parse_overrides(["+expt=dc_gan", plus + "kid_on_device=true"])[3]
        assert run["kid_on_device"] is True
    assert parse_overrides(["+expt=dc_gan"])[3]["kid_on_device"] is False


def test_evaluate_keeps_the_host_path_by_default():
    import inspect

    from lightning_gan_zoo_amd import eval as E
    assert inspect.signature(E.evaluate).parameters["kid_on_device"].default is False
    assert list(inspect.signature(E.evaluate).parameters)[:5] == ["module", "dump", "feature_fn", "real_act", "n_subsets"]
