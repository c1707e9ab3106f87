"""Generator weight averaging, the parts that need no GPU: the two runner keys, the C-ABI declarations and the
host-side job fill call (it touches no device, so its error codes are checked here)."""
import ctypes

import pytest

from lightning_gan_zoo_amd import _lib

BAD_SHAPE, TOO_LARGE = -1, -5
CHUNK = 4096


def test_runner_keys_default_to_off_with_gan_stabilitys_beta():
    from lightning_gan_zoo_amd.run_network import RUNNER_KEYS
    assert RUNNER_KEYS["generator_average"] is False
    assert RUNNER_KEYS["generator_average_beta"] == 0.999          # gan_stability's model_average_beta default


@pytest.mark.parametrize("plus", ["", "+"])
def test_parse_overrides_accepts_both_keys(plus):
    from lightning_gan_zoo_amd.run_network import parse_overrides
    conf, expt, rest, run = parse_overrides(["+expt=dc_gan", plus + "generator_average=true",
                                             plus + "generator_average_beta=0.99", "train.batch_size=4"])
    assert conf is None and expt == "dc_gan"
    assert run["generator_average"] is True and run["generator_average_beta"] == 0.99
    assert rest == ["+expt=dc_gan", "train.batch_size=4"]          # runner keys never reach the config composer
    _, _, _, run = parse_overrides(["+expt=dc_gan"])
    assert run["generator_average"] is False and run["generator_average_beta"] == 0.999


def test_symbols_are_declared_and_resolve():
    protos = _lib.parse_header()
    assert protos["gz_ema_job_bytes"] == (ctypes.c_size_t, [])
    assert protos["gz_ema_job"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_longlong, ctypes.c_int])
    assert protos["gz_ema_update"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                                      ctypes.c_float, ctypes.c_void_p])
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gz_ema_job_bytes", "gz_ema_job", "gz_ema_update"):
        assert hasattr(dll, name), name
    assert _lib.lib.gz_ema_job_bytes() >= 2 * ctypes.sizeof(ctypes.c_void_p) + 8 + 4


def _fill(avg, src, numel, first_block=0, job=True):
    lib = _lib.lib
    buf = (ctypes.c_char * lib.gz_ema_job_bytes())()
    return lib.gz_ema_job(buf if job else None, ctypes.c_void_p(avg), ctypes.c_void_p(src), numel, first_block), bytes(buf)


def test_job_fill_returns_the_block_count():
    """Addresses are only recorded, never dereferenced: made-up ones do."""
    a, s = 0x10000000, 0x20000000
    for numel, blocks in ((1, 1), (CHUNK - 1, 1), (CHUNK, 1), (CHUNK + 1, 2), (2 * CHUNK + 2, 3), (0, 0)):
        assert _fill(a, s, numel)[0] == blocks, numel
    assert _fill(0, 0, 0)[0] == 0                                  # an empty tensor has no address: a job without blocks
    # the record differs where the recorded values differ: alignment class, prefix
    assert _fill(a, s, 8)[1] != _fill(a + 4, s, 8)[1]
    assert _fill(a, s, 8, 0)[1] != _fill(a, s, 8, 5)[1]
    assert _fill(a, s, 8)[1] == _fill(a, s, 8)[1]


def test_job_fill_error_codes():
    a, s = 0x10000000, 0x20000000
    assert _fill(0, s, 16)[0] == BAD_SHAPE                          # null avg
    assert _fill(a, 0, 16)[0] == BAD_SHAPE                          # null src
    assert _fill(a, s, 16, job=False)[0] == BAD_SHAPE               # null record
    assert _fill(a, s, -1)[0] == BAD_SHAPE                          # negative numel
    assert _fill(a, s, 16, first_block=-1)[0] == BAD_SHAPE
    assert _fill(a, a, 16)[0] == BAD_SHAPE                          # the same array
    assert _fill(a, a + 60, 16)[0] == BAD_SHAPE                     # src starts inside avg's last element
    assert _fill(a + 60, a, 16)[0] == BAD_SHAPE                     # avg starts inside src
    assert _fill(a, a + 64, 16)[0] == 1                             # adjacent, not overlapping
    assert _fill(a + 64, a, 16)[0] == 1
    assert _fill(a, s, 16, first_block=0x7fffffff)[0] == TOO_LARGE  # the grid index would not fit an int


def test_update_rejects_bad_arguments_before_any_launch():
    """count and total_blocks are validated on the host; nothing reaches the device (there is none here)."""
    lib = _lib.lib
    table = (ctypes.c_char * lib.gz_ema_job_bytes())()
    assert lib.gz_ema_update(None, 1, 1, 0.5, 0.5, None) == BAD_SHAPE
    assert lib.gz_ema_update(table, 0, 1, 0.5, 0.5, None) == BAD_SHAPE
    assert lib.gz_ema_update(table, -3, 1, 0.5, 0.5, None) == BAD_SHAPE
    assert lib.gz_ema_update(table, 1, -1, 0.5, 0.5, None) == BAD_SHAPE
