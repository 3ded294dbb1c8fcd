"""The split JPEG entropy decode on the host (K18): omr_jpeg_decode_host_split -- plain loops that
play the lanes of k_jpeg_entropy_split through guess, settle, scan and write with the per-lane
decoder the kernel uses, then the DC sums -- against the serial decoder omr_jpeg_decode_host, byte
for byte and status for status, on every stream of tests/golden/tiff_jpeg.npz and
tests/golden/jpeg_split.npz, on good variants, and on damaged and truncated copies.  The stats
prove that the inputs reach several rounds, slow settling and a subsequence that begins on a
stuffed 00."""
import numpy as np
import pytest

import jpeg_split_cases as sc
import omr
import tiff_jpeg_cases as jc
from omr import _lib

BITS = (32, 64, 256, 1024)
LANES = (1, 4, 256)


@pytest.fixture(scope="module")
def reference():
    """The serial decoder's bytes of every stream, decoded once."""
    out = {}
    for s in sc.ALL:
        st, px = sc.serial(s)
        assert st == _lib.OK, s.id
        out[s.id] = px
    return out


def test_fixture_pixels_are_the_serial_decoders(reference):
    for s in sc.SPLIT:
        assert reference[s.id] == np.ascontiguousarray(sc.split_pixels(s.id)).tobytes(), s.id
    assert {"noise420", "noise444_q100", "flat420", "noise422", "grey", "noise420_rst"} <= set(sc.SPLIT_NAMES)
    for s in sc.SPLIT:
        assert ("RESTART" in omr.jpeg_stream_forms(s.data)) == (s.id == "noise420_rst"), s.id


@pytest.fixture(scope="module")
def all_stats(reference):
    """{(id, bits, lanes): stats}, with the bytes of every decode compared on the way."""
    out = {}
    for s in sc.ALL:
        for bits in BITS:
            for lanes in LANES:
                st, px, stats = sc.split(s, bits, lanes)
                assert st == _lib.OK and px == reference[s.id], (s.id, bits, lanes)
                out[(s.id, bits, lanes)] = stats
    return out


def test_split_equals_serial_on_every_stream(all_stats):
    assert len(all_stats) == len(sc.ALL) * len(BITS) * len(LANES) and len(sc.ALL) > 50


def test_stats_show_the_hard_cases(all_stats):
    # several rounds of 256 lanes: at 32 bits a stream above 1 KiB has more than 256 subsequences
    many = [k for k, v in all_stats.items() if k[2] == 256 and v["rounds"] >= 2]
    assert any(k[0].startswith("rgb_strips") for k in many) and any(k[0] == "noise420" for k in many), many
    # a single lane never settles; the subsequences cover the interval's bits
    for (ident, bits, lanes), v in all_stats.items():
        if lanes == 1:
            assert v["max_settle_iterations"] == 0 and v["redecodes"] == 0 and v["rounds"] <= v["subsequences"]
    # guessed states that take several iterations to settle.  (The flat tile does not supply them: an
    # MCU of it is 32 bits -- four times 00 1010, twice 00 00 -- so at every S here a subsequence begins
    # on an MCU and every guess is right.  The noise tiles do: a guess is off by its block and its zigzag index.)
    assert max(v["max_settle_iterations"] for k, v in all_stats.items() if k[0] == "flat420") == 0
    slow = [k for k, v in all_stats.items() if v["max_settle_iterations"] >= 3]
    assert any(k[0] == "noise420" for k in slow) and any(k[0] == "grey" for k in slow), len(slow)
    s = sc.split_stream("noise420")
    first, end = sc.entropy_span(s.data)
    assert all_stats[("noise420", 1024, 256)]["subsequences"] == (8 * (end - first) + 1023) // 1024


def test_a_subsequence_begins_on_a_stuffed_zero(reference):
    """Found by position: an FF 00 whose 00 is the first raw byte of a subsequence."""
    met = 0
    for s in sc.SPLIT:
        if s.id == "noise420_rst":
            continue
        first, end = sc.entropy_span(s.data)
        body = s.data[first:end]
        for bits in BITS:
            at = [p for p in range(1, len(body)) if body[p] == 0 and body[p - 1] == 0xFF and (8 * p) % bits == 0]
            if at:
                met += 1
                for lanes in (4, 256):
                    st, px, _ = sc.split(s, bits, lanes)
                    assert st == _lib.OK and px == reference[s.id], (s.id, bits, lanes, at[0])
    assert met >= 3


def pad_cleared(data, j):
    """The low j bits of the last entropy-coded byte set to zeros; None where that byte is a stuffed 00 or they are not all ones."""
    first, end = sc.entropy_span(data)
    b = data[end - 1]
    if (b == 0 and data[end - 2] == 0xFF) or (b & ((1 << j) - 1)) != (1 << j) - 1:
        return None
    return data[:end - 1] + bytes([b & ~((1 << j) - 1) & 255]) + data[end:]


def test_good_variants_are_accepted_alike(reference):
    checked = 0
    for s in sc.SPLIT + [sc.tiff_streams(n)[1] for n in ("grey_strips", "ycc420_tiles", "rgb_strips")]:
        if "RESTART" in omr.jpeg_stream_forms(s.data, s.tables):
            continue
        has_pad = "PAD_BITS" in omr.jpeg_stream_forms(s.data, s.tables)
        for j in range(1, 8):
            v = pad_cleared(s.data, j)
            if v is None:
                break
            want = sc.serial(s, v)
            if j == 1 and has_pad:
                assert want == (_lib.OK, reference[s.id]), s.id     # the last bit of a padded byte is a pad bit
                checked += 1
            for bits, lanes in ((32, 256), (1024, 4)):
                assert sc.split(s, bits, lanes, v)[:2] == want, (s.id, j, bits, lanes)
        # two surplus 00 bytes before EOI: the serial decoder never looks at them (it stops at the frame's last block)
        first, end = sc.entropy_span(s.data)
        v = s.data[:end] + b"\0\0" + s.data[end:]
        want = sc.serial(s, v)
        assert want == (_lib.OK, reference[s.id]), s.id
        for bits, lanes in ((32, 256), (64, 3), (1024, 4)):
            assert sc.split(s, bits, lanes, v)[:2] == want, (s.id, bits, lanes)
    assert checked >= 4


@pytest.mark.parametrize("variant", [jc.as_progressive, jc.as_12bit, jc.as_two_scans, jc.with_wrong_frame_size,
                                     jc.with_undefined_code, jc.with_swapped_rst],
                         ids=["progressive", "12bit", "two-scans", "frame", "code", "rst"])
def test_tiff_jpeg_variants_get_the_serial_status(variant):
    pool = [sc.tiff_streams("ycc420_rst_q30")[1], sc.split_stream("noise420_rst")] if variant is jc.with_swapped_rst else \
        [sc.tiff_streams("ycc420_tiles")[1], sc.tiff_streams("grey_strips")[1], sc.split_stream("noise422"), sc.split_stream("grey")]
    for s in pool:
        v = variant(s.data)
        want = sc.serial(s, v)
        assert want[0] != _lib.OK
        for bits, lanes in ((32, 256), (256, 4), (1024, 1)):
            assert sc.split(s, bits, lanes, v)[:2] == want, (s.id, bits, lanes)


def test_flipped_bytes_get_the_serial_status():
    rng = np.random.default_rng(18)
    kinds = set()
    for s in (sc.split_stream("noise422"), sc.split_stream("noise420_rst"), sc.tiff_streams("ycc420_tiles")[0]):
        first = jc.sos_at(s.data)
        for p in rng.integers(first, len(s.data) - 2, 200 if s.id == "noise422" else 40):
            v = bytearray(s.data)
            v[p] ^= int(rng.integers(1, 256))
            want = sc.serial(s, bytes(v))
            kinds.add(want[0])
            for bits, lanes in ((32, 256), (1024, 4)):
                assert sc.split(s, bits, lanes, bytes(v))[:2] == want, (s.id, int(p), bits, lanes)
    assert kinds == {_lib.OK, _lib.INTERNAL}               # some damage still decodes (to the same wrong pixels), some does not


def test_every_truncation_gets_the_serial_status():
    s = sc.split_stream("grey")
    for cut in range(1, len(s.data)):
        want = sc.serial(s, s.data[:cut])
        assert want[0] == _lib.INTERNAL
        for bits, lanes in ((32, 256), (1024, 4)):
            assert sc.split(s, bits, lanes, s.data[:cut])[:2] == want, (cut, bits, lanes)
    # a cut stream never passes the header parser (no EOI).  With an EOI behind the cut it does, and
    # the interval runs out of bits inside the entropy decode
    first, end = sc.entropy_span(s.data)
    for cut in range(first, end):
        v = s.data[:cut] + b"\xff\xd9"
        want = sc.serial(s, v)
        assert want[0] == _lib.INTERNAL, cut
        for bits, lanes in ((32, 256), (1024, 4)):
            assert sc.split(s, bits, lanes, v)[:2] == want, (cut, bits, lanes)


def test_arguments():
    s = sc.split_stream("grey")
    for bits, lanes in ((0, 4), (16, 4), (48, 4), (4128, 4), (1024, 0), (1024, 257)):
        assert sc.split(s, bits, lanes)[0] == _lib.INVALID_ARGUMENT, (bits, lanes)
    assert sc.split(s, 4096, 256)[:2] == sc.serial(s)
    stats = _lib.JpegSplitStats()
    assert _lib.lib.omr_jpeg_decode_host_split(None, 0, None, 4, 8, 8, 1, 0, 1024, 4, None, _lib.ctypes.byref(stats)) == _lib.INVALID_ARGUMENT
