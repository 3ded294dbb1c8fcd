"""JPEG and JPEG 2000 reads and batch decodes interleaved on one context (K17, K19): the two codecs
share the image-codec tail of the device-read pipeline, the staging of the batch entry points and
the status fetch, and nothing a call leaves behind may reach the next.  In this order: read_regions
on a JPEG file, on a JPEG 2000 file, jpeg_decode_batch_device with a truncated stream (refused on
the host) and one with an undefined code (refused by K17a: its status comes back from the device)
beside a good one, the JPEG read again, j2k_decode_batch_device with a truncated stream, the
JPEG 2000 read again.  Every read equals get_tile of the same region byte for byte, with canaries
behind the region; every batch result and status equals the host decoder's.

The files are the smallest of tests/golden/tiff_jpeg.npz and tiff_j2k.npz whose level is at least
two segments wide, a grey one where there is one (the JPEG fixture's only grey file is in strips, so
its file is a chunky one and the read takes one channel).  The region of 40 x 24 samples straddles a
segment corner: four segments, four placements."""
import pytest

import omr
import tiff_j2k_cases as j2
import tiff_jpeg_cases as jp
from omr import _lib
from test_tiff_codecs_gpu import CANARY, read_checked

pytestmark = pytest.mark.gpu

W, H = 40, 24


def smallest_two_wide(cases, names, tmp):
    """(name, x, y): the smallest file at least two segments wide and two down, grey before chunky,
    and the origin of a W x H region around the first inner segment corner."""
    found = []
    for name in names:
        n = cases.pixels(name).shape[0]
        with omr.TiffImage(cases.write(tmp, name), 1, n, 1, accept=cases.ACCEPT) as img:
            sw, sh = img.info["segment_width"], img.info["segment_height"]
            if img.info["tiled"] and sw < img.size_x and sh < img.size_y:
                found.append((n > 1, len(cases.raw(name)), name, sw - W // 2, sh - H // 2))
    assert found
    return min(found)[2:]


def host_status(decode):
    try:
        return _lib.OK, decode()
    except omr.OmrError as e:
        return e.status, None


def test_reads_and_batches_interleaved_on_one_context(ctx, tmp_path):
    jpeg_name, jx, jy = smallest_two_wide(jp, jp.NAMES, tmp_path)
    j2k_name, kx, ky = smallest_two_wide(j2, j2.FILES, tmp_path)
    assert j2.pixels(j2k_name).shape[0] == 1

    def read_equals_get_tile(img, x, y):
        got = read_checked(ctx, img, 0, [(0, 0, 0, x, y)], W, H)
        want = img.get_tile(0, 0, 0, 0, x, y, W, H)
        assert want.shape == (H, W) and got[0].tobytes() == want.tobytes()

    tables, segs, n, ycc = jp.streams_of(jpeg_name)
    _, _, w, h, good = segs[0]
    jpeg_streams = [good, good[:len(good) // 2], jp.with_undefined_code(good)]
    jpeg_host = [host_status(lambda s=s: omr.jpeg_decode_host(s, w, h, n, ycc, tables)) for s in jpeg_streams]
    assert [st for st, _ in jpeg_host] == [_lib.OK, _lib.INTERNAL, _lib.INTERNAL]

    stream_name = "grey_41x37_cb4"
    kw, kh, ks, kbits = j2.shape_of(stream_name)
    s = j2.stream(stream_name)
    j2k_streams = [s[:len(s) // 2], s]
    j2k_host = [host_status(lambda s=s: omr.j2k_decode_host(s, kw, kh, ks, kbits)) for s in j2k_streams]
    assert [st for st, _ in j2k_host] == [_lib.INTERNAL, _lib.OK]

    with omr.TiffImage(jp.write(tmp_path, jpeg_name), 1, n, 1, accept=jp.ACCEPT) as jpeg, \
            omr.TiffImage(j2.write(tmp_path, j2k_name), 1, 1, 1, accept=j2.ACCEPT) as j2k:
        read_equals_get_tile(jpeg, jx, jy)
        read_equals_get_tile(j2k, kx, ky)

        got, status = omr.jpeg_decode_batch_device(ctx, jpeg_streams, [(w, h)] * len(jpeg_streams), n, ycc, tables)
        assert status == [st for st, _ in jpeg_host]
        assert got[0].tobytes() == jpeg_host[0][1].tobytes()
        assert (got[1] == CANARY).all()                      # a stream refused on the host is never decoded

        read_equals_get_tile(jpeg, jx, jy)                   # no status of the batch reaches this read

        got, status = omr.j2k_decode_batch_device(ctx, j2k_streams, [(kw, kh)] * 2, ks, kbits)
        assert status == [st for st, _ in j2k_host]
        assert got[1].dtype == j2k_host[1][1].dtype and got[1].tobytes() == j2k_host[1][1].tobytes()
        assert (got[0] == CANARY).all()

        read_equals_get_tile(j2k, kx, ky)
