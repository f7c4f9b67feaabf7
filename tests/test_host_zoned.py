"""The red-zone checker of tests/zoned.py on NumPy buffers (no GPU): an instrument that cannot fail proves nothing, so
every planted write must be reported at the offset it was planted at, and an intact buffer must pass.  Also: every
compute export of include/vqvae_hip.h has a row in the contract table of tests/test_gpu_abi_contract.py, and the tests a row
names exist there or in tests/test_gpu_abi_contract_chain.py."""
import os
import re

import numpy as np
import pytest

import zoned as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _image(payload_bytes, shift=0, zone=512):
    lay = Z.Layout(payload_bytes, zone, shift)
    payload = (np.arange(payload_bytes) % 251).astype(np.uint8)
    return lay, Z.make_image(lay, payload), payload


@pytest.mark.parametrize('payload_bytes,shift', [(4000, 0), (4, 0), (1022, 4), (6, 2), (4096, 12)])
def test_intact_buffer_passes_and_payload_is_in_place(payload_bytes, shift):
    lay, img, payload = _image(payload_bytes, shift)
    assert lay.start % 256 == shift and lay.total % 4 == 0 and lay.total - lay.end >= lay.zone_bytes
    assert Z.find_corruption(lay, img) == []
    np.testing.assert_array_equal(img[lay.start:lay.end], payload)
    # any content of the payload is the callee's business
    img[lay.start:lay.end] = 0xff
    assert Z.find_corruption(lay, img) == []


@pytest.mark.parametrize('payload_bytes,shift', [(4000, 0), (1022, 4), (6, 2)])
@pytest.mark.parametrize('where', ['byte_before', 'byte_after', 'far_front', 'far_back'])
def test_planted_write_is_reported_at_its_offset(payload_bytes, shift, where):
    lay, img, _ = _image(payload_bytes, shift)
    pos = {'byte_before': lay.start - 1, 'byte_after': lay.end, 'far_front': 0, 'far_back': lay.total - 1}[where]
    img[pos] ^= 0x40
    found = Z.find_corruption(lay, img, 'y')
    assert len(found) == 1
    c = found[0]
    assert c.zone == ('front' if pos < lay.start else 'back')
    assert c.first == c.last == pos - lay.start and c.count == 1
    assert {'byte_before': c.first == -1, 'byte_after': c.first == payload_bytes,
            'far_front': c.first == -lay.start, 'far_back': c.first == lay.total - 1 - lay.start}[where]
    word = int(img.view('<u4')[pos // 4])
    assert c.first_word == word and ('0x%08x' % word) in str(c) and 'y: ' in str(c)


def test_a_run_of_stores_reports_first_and_last():
    lay, img, _ = _image(1000)
    img[lay.end + 8:lay.end + 24] = 0          # four floats behind the payload
    img[lay.start - 4:lay.start] = 0           # one float in front of it
    found = {c.zone: c for c in Z.find_corruption(lay, img)}
    assert (found['back'].first, found['back'].last) == (1000 + 8, 1000 + 23)
    assert (found['front'].first, found['front'].last) == (-4, -1) and found['front'].first_word == 0


def test_a_copy_of_the_neighbouring_zone_is_caught():
    """The pattern depends on the position: a kernel that copies what lies 16 B further into the zone changes it."""
    lay, img, _ = _image(1000)
    img[lay.end:lay.end + 16] = img[lay.end + 16:lay.end + 32].copy()
    assert Z.find_corruption(lay, img)[0].first == 1000
    words = Z.pattern_bytes(lay).view('<f4')
    assert np.isnan(words).all() and len(set(Z.pattern_bytes(lay).view('<u4').tolist())) == lay.total // 4


def test_index_zones_hold_valid_indices_that_differ_from_their_neighbours():
    lay = Z.Layout(400, 512)
    pat = Z.index_pattern_bytes(lay, 0, 50).view('<i4')
    assert pat.min() >= 0 and pat.max() < 50 and (pat[1:] != pat[:-1]).all()
    img = Z.make_image(lay, np.zeros(400, np.uint8), Z.index_pattern_bytes(lay, 0, 50))
    assert Z.find_corruption(lay, img, zone_pattern=Z.index_pattern_bytes(lay, 0, 50)) == []
    img[lay.end] ^= 1
    assert Z.find_corruption(lay, img, zone_pattern=Z.index_pattern_bytes(lay, 0, 50))[0].first == 400


def test_poison_is_nan_as_float_and_out_of_range_as_index():
    p = Z.poison_payload(10)
    assert p.size == 10 and np.isnan(p[:8].view('<f4')).all() and (p[:8].view('<i4') > (1 << 30)).all()


# ---- the contract table covers the header ------------------------------------------------------------------------
PLUMBING = re.compile(r'^vqvae_(last_error_string|abi_version|device_|set_|get_|malloc|free|memcpy|memset|host_|stream_|'
                      r'event_|prof_|comm_|graph_)')


def header_exports():
    text = open(os.path.join(ROOT, 'include', 'vqvae_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(vqvae_[a-z0-9_]+)\s*\(', text)))


def test_every_compute_export_has_a_contract_row():
    import test_gpu_abi_contract as T
    import test_gpu_abi_contract_chain as TC
    exports = header_exports()
    from vqvae_amd import _lib
    assert set(exports) == set(_lib.PROTOTYPES), set(exports) ^ set(_lib.PROTOTYPES)       # 127 symbols
    compute = [e for e in exports if not PLUMBING.match(e)]
    missing = [e for e in compute if e not in T.CONTRACTS]
    assert not missing, 'compute exports without a row in tests/test_gpu_abi_contract.py CONTRACTS: %s' % missing
    stale = [e for e in T.CONTRACTS if e not in compute]
    assert not stale, 'rows of CONTRACTS that name no compute export: %s' % stale
    for name, row in T.CONTRACTS.items():
        assert set(row) == {'zones', 'inputs_only', 'maxima', 'init'}, name
        # a row that claims a contract names the test that applies it, and that test exists
        for key in ('zones', 'inputs_only', 'maxima'):
            for test in row[key]:
                assert callable(getattr(T, test, None)) or callable(getattr(TC, test, None)), \
                    '%s: %s names %s, which is in neither module' % (name, key, test)
