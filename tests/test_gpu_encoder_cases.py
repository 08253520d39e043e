"""GPU encoder (include/pcr_gpu_encode.h) against the CPU encoder on the inputs of tests/encoder_cases.py, where the encoder's own
rules decide: equal Morton keys (the dropped X bit 31 among them), leaf-against-internal ties of the Huffman construction, shared
escape keys, chains without a partial word, the shortest chain beside the longest in one cluster, chunk edges and constructed
colour blocks. tests/test_encoder_cases_cpu.py proves without a GPU that every input is what it claims; here the `.huffman` image
and the statistics must be the CPU encoder's, byte for byte, plain and with padded tails. A mismatch names the batch and the first
section of its record that differs (encoder_cases.first_difference), so that the stage at fault can be read off the failure."""
import ctypes as C

import numpy as np
import pytest

import pcrhpg24_amd as P
from tests import decoder_cases as D
from tests import encoder_cases as E

pytestmark = pytest.mark.gpu

PCR_E_ARG = -1
PADS = [pytest.param(False, id="plain"), pytest.param(True, id="padded")]


@pytest.fixture(scope="module")
def ctx():
    c = P.Context(0)
    yield c
    c.close()


def gpu_image(ctx, name, pad, **override):
    x, y, z, c, las, kw = E.case(name)
    image, st = ctx.gpu_encode_points(x, y, z, c, las, pad_tails=pad, **{**kw, **override})
    return bytes(image.view()), st


def check(ctx, name, pad, **override):
    want, st_want = E.cpu_image(name, pad)
    got, st_got = gpu_image(ctx, name, pad, **override)
    assert got == want, f"{name} {'padded' if pad else 'plain'}: {E.first_difference(want, got)}"
    assert st_got == st_want
    return got


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", [n for n in E.CASES if not n.startswith("dec_")])
def test_case(ctx, name, pad):
    check(ctx, name, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", D.STREAMS)
def test_decoder_stream(ctx, name, pad):
    """The image is the very stream tests/test_gpu_decoder.py decodes."""
    got = check(ctx, f"dec_{name}", pad)
    want = bytes(E.decoder_stream(name, pad))
    assert got == want, E.first_difference(want, got)


def test_default_chunk_points(ctx):
    """One chunk of the default 100 batches: the image of a single batch does not depend on the scratch it was given."""
    check(ctx, "two_symbols", False, chunk_points=0)


def test_calls_do_not_leave_state_behind(ctx):
    """Scratch and the error word are per call: the same image twice, with another input's in between."""
    for name, pad in (("key_ties", True), ("two_symbols", True), ("key_ties", True), ("mixed_lanes", False), ("fib", False)):
        check(ctx, name, pad)


def raw_call(ctx, flags, las):
    x, y, z, c, _, _ = E.case("n1")
    out, ln, st = C.c_void_p(0x1234), C.c_size_t(77), P.host.EncodeStats()
    rc = ctx.lib.pcr_gpu_encode_points(ctx.h, x.ctypes.data, y.ctypes.data, z.ctypes.data, c.ctypes.data, len(x), las, flags, E.CHUNK,
                                       C.byref(out), C.byref(ln), C.byref(st))
    return rc, out.value, ln.value, ctx.lib.pcr_last_error(ctx.h) or b""


def test_refusals(ctx):
    las = E.case("n1")[4]
    for flags, header, word in ((1 | 4, C.byref(las), b"BC7"), (1, None, b"null")):
        rc, out, ln, message = raw_call(ctx, flags, header)
        assert rc == PCR_E_ARG and word in message, (rc, message)
        assert out == 0x1234 and ln == 77, "a refused call writes nothing"
    check(ctx, "n1", False)                                                     # and the context encodes as before
