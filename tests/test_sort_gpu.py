"""GPU: ssdk_sort_pairs_u64 (the stable 8-bit LSD radix sort of csrc/metrics.hip) against np.argsort(kind='stable'): keys AND values
exactly equal, at the sizes around its tiling constants -- lanes of 64, wave quarters of 1024, tiles of 4096 keys, row-scan rounds of
256 tiles, the doubled tile above 4096 tiles -- and at every digit count."""
import time

import numpy as np
import pytest
import torch

from single_shot_detection_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 5121, 12289 + 37]   # 5121: one key in wave 1 of tile 1; 4097: waves 1-3 of the last tile empty
END_BITS = [8, 9, 16, 37, 40, 64]                                                # 1, 2, 2, 5, 5, 8 digits: odd pass counts, and the top digit sorted once more
PATTERNS = ['random', 'all_equal', 'two_keys', 'ascending', 'descending', 'top_digit_only', 'digit_constant_per_64']
KEY_SENTINEL, VAL_SENTINEL = -0x0123456789ABCDF0, -0x1234567
E_INVALID, E_WORKSPACE = -1, -2


def random_keys(rng, n, end_bit):
    return rng.integers(0, (1 << end_bit) - 1, n, dtype=np.uint64, endpoint=True)


def make_keys(pattern, rng, n, end_bit):
    digits = (end_bit + 7) // 8
    top_shift, top_bits = 8 * (digits - 1), end_bit - 8 * (digits - 1)
    if pattern == 'random':
        return random_keys(rng, n, end_bit)
    if pattern == 'all_equal':       # vals_out must come back in input order: stability across lanes, waves and tiles
        return np.full(n, random_keys(rng, 1, end_bit)[0], np.uint64)
    if pattern == 'two_keys':
        return random_keys(rng, 2, end_bit)[rng.integers(0, 2, n)]
    if pattern == 'ascending':
        return np.sort(random_keys(rng, n, end_bit))
    if pattern == 'descending':
        return np.sort(random_keys(rng, n, end_bit))[::-1].copy()
    if pattern == 'top_digit_only':
        low = random_keys(rng, 1, end_bit)[0] & np.uint64((1 << top_shift) - 1)
        return low | (rng.integers(0, 1 << top_bits, n, dtype=np.uint64) << np.uint64(top_shift))
    if pattern == 'digit_constant_per_64':   # every digit is the same inside a group of 64 consecutive keys (one ballot round) and differs between groups
        group = np.arange(n, dtype=np.uint64) // np.uint64(64)
        key = np.zeros(n, np.uint64)
        for d in range(digits):
            key |= ((group * np.uint64(37 + 2 * d) + np.uint64(11 * d + 5)) & np.uint64(255)) << np.uint64(8 * d)
        return key & np.uint64((1 << end_bit) - 1)
    raise KeyError(pattern)


def device_sort(keys, vals, end_bit, n=None, ws_bytes=None, no_ws=False):
    """-> (status, keys_out, vals_out, keys_after, vals_after) as numpy; the outputs are pre-filled with a sentinel"""
    lib = _lib.lib()
    n = len(keys) if n is None else n
    k = torch.from_numpy(keys.view(np.int64)).cuda()
    v = torch.from_numpy(vals.view(np.int32)).cuda()
    ko, vo = torch.full_like(k, KEY_SENTINEL), torch.full_like(v, VAL_SENTINEL)
    need = lib.ssdk_sort_pairs_u64_workspace_bytes(n)
    ws = torch.empty((max(need, 256),), dtype=torch.uint8, device='cuda')
    rc = lib.ssdk_sort_pairs_u64(_lib.ptr(k), _lib.ptr(v), n, end_bit, _lib.ptr(ko), _lib.ptr(vo), None if no_ws else _lib.ptr(ws),
                                 need if ws_bytes is None else ws_bytes, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, ko.cpu().numpy().view(np.uint64), vo.cpu().numpy().view(np.uint32), k.cpu().numpy().view(np.uint64), v.cpu().numpy().view(np.uint32)


def check_sort(keys, vals, end_bit, tag):
    t0 = time.perf_counter()
    perm = np.argsort(keys, kind='stable')
    host = time.perf_counter() - t0
    rc, ko, vo, ka, va = device_sort(keys, vals, end_bit)
    assert rc == 0, (tag, rc, _lib.lib().ssdk_last_error_string())
    assert np.array_equal(ko, keys[perm]), tag
    assert np.array_equal(vo, vals[perm]), tag
    assert np.array_equal(ka, keys) and np.array_equal(va, vals), tag   # the inputs are staged, not clobbered (include/ssdk.h)
    return host


@pytest.mark.parametrize('end_bit', END_BITS)
@pytest.mark.parametrize('pattern', PATTERNS)
def test_sort_pairs_around_the_tiling_constants(pattern, end_bit):
    rng = np.random.default_rng(1000 * PATTERNS.index(pattern) + end_bit)
    for n in SIZES:
        keys = make_keys(pattern, rng, n, end_bit)
        assert keys.dtype == np.uint64 and len(keys) == n and (end_bit == 64 or int(keys.max()) < (1 << end_bit))
        vals = rng.permutation(n).astype(np.uint32)           # not arange: a key / value mix-up shows
        check_sort(keys, vals, end_bit, (pattern, end_bit, n))


def test_sort_ignores_bits_at_and_above_end_bit_and_sorts_in_place():
    rng = np.random.default_rng(7)
    n, end_bit = 5121, 20
    keys = random_keys(rng, n, 64)
    vals = rng.permutation(n).astype(np.uint32)
    perm = np.argsort(keys & np.uint64((1 << end_bit) - 1), kind='stable')
    rc, ko, vo, _, _ = device_sort(keys, vals, end_bit)
    assert rc == 0 and np.array_equal(ko, keys[perm]) and np.array_equal(vo, vals[perm])
    # keys_out == keys and vals_out == vals: allowed, the inputs are staged in the workspace first
    lib = _lib.lib()
    k, v = torch.from_numpy(keys.view(np.int64)).cuda(), torch.from_numpy(vals.view(np.int32)).cuda()
    ws = torch.empty((lib.ssdk_sort_pairs_u64_workspace_bytes(n),), dtype=torch.uint8, device='cuda')
    assert lib.ssdk_sort_pairs_u64(_lib.ptr(k), _lib.ptr(v), n, end_bit, _lib.ptr(k), _lib.ptr(v), _lib.ptr(ws), ws.numel(), _lib.current_stream()) == 0
    assert np.array_equal(k.cpu().numpy().view(np.uint64), keys[perm]) and np.array_equal(v.cpu().numpy().view(np.uint32), vals[perm])


def test_sort_second_rowscan_round():
    """258 tiles: radix_rowscan_kernel walks 256 tiles per round, so tiles 256 and 257 take a second round with a non-zero carry"""
    n = 256 * 4096 + 4096 + 7
    assert (n + 4095) // 4096 == 258
    rng = np.random.default_rng(11)
    host = check_sort(random_keys(rng, n, 40), rng.permutation(n).astype(np.uint32), 40, 'rowscan')
    assert host < 5.0


def test_sort_doubled_tile():
    """4096 * 4096 + 1 keys: more than 4096 tiles of 4096, so the tile doubles to 8192 keys and the wave quarters to 2048.  16-bit keys
    keep the host's stable argsort a radix sort."""
    n = 4096 * 4096 + 1
    rng = np.random.default_rng(12)
    keys16 = rng.integers(0, 1 << 16, n, dtype=np.uint16)
    t0 = time.perf_counter()
    perm = np.argsort(keys16, kind='stable')
    host = time.perf_counter() - t0
    keys, vals = keys16.astype(np.uint64), rng.permutation(n).astype(np.uint32)
    rc, ko, vo, _, _ = device_sort(keys, vals, 16)
    assert rc == 0
    assert np.array_equal(ko, keys[perm]) and np.array_equal(vo, vals[perm])
    assert host < 5.0, host


def test_sort_refusals_write_nothing():
    lib = _lib.lib()
    rng = np.random.default_rng(13)
    n = 4097
    keys, vals = random_keys(rng, n, 32), rng.permutation(n).astype(np.uint32)
    need = lib.ssdk_sort_pairs_u64_workspace_bytes(n)
    assert need >= n * 12 and lib.ssdk_sort_pairs_u64_workspace_bytes(-1) == 0 and lib.ssdk_sort_pairs_u64_workspace_bytes(1 << 31) == 0
    for kw, code in ((dict(n=-1), E_INVALID), (dict(n=1 << 31), E_INVALID), (dict(end_bit=0), E_INVALID), (dict(end_bit=65), E_INVALID),
                     (dict(end_bit=-8), E_INVALID), (dict(ws_bytes=need - 1), E_WORKSPACE), (dict(ws_bytes=0), E_WORKSPACE),
                     (dict(no_ws=True), E_WORKSPACE)):
        args = dict(end_bit=32)
        args.update(kw)
        rc, ko, vo, ka, va = device_sort(keys, vals, **args)
        assert rc == code, (kw, rc)
        assert b'ssdk_sort_pairs_u64' in lib.ssdk_last_error_string()
        assert np.all(ko.view(np.int64) == KEY_SENTINEL) and np.all(vo.view(np.int32) == VAL_SENTINEL), kw
        assert np.array_equal(ka, keys) and np.array_equal(va, vals)
    rc, ko, vo, _, _ = device_sort(keys, vals, 32, n=0)        # nothing to sort: accepted, nothing written
    assert rc == 0 and np.all(ko.view(np.int64) == KEY_SENTINEL) and np.all(vo.view(np.int32) == VAL_SENTINEL)
