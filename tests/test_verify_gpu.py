"""The Decoder's verified mode (vpcc_decoder_set_verify): clean streams pass every check with no false alarm, and a frame
corrupted at ingest, reconstruction or delivery (VPCC_DECODER_TEST_CORRUPT, a test-only hook that alters data) is never
handed over — the stream ends in front of it with an error that names the stage and the frame."""
import os
import tempfile
import zlib

import numpy as np
import pytest

import digest_ref
import oracle_binding as ob
from tmc2rs import container, recon, synth

pytestmark = pytest.mark.gpu


def _crc(xyz, rgb):
    return zlib.crc32(np.ascontiguousarray(rgb).tobytes(), zlib.crc32(np.ascontiguousarray(xyz).tobytes()))


@pytest.fixture(scope="module")
def longdress32():
    frames = [synth.longdress_frame(i) for i in range(32)]
    ref = []
    for f in frames:
        st, r = ob.reconstruct(f)
        assert st == 0 and r["n"] > 0
        ref.append((r["n"], _crc(ob.xyz_array(r), ob.rgb_array(r))))
    return frames, ref


def _stream(gofs, devices=(0,), verify="all"):
    """[(n, crc, digest, frame digest by digest_ref)], error, verify stats."""
    d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    path = os.path.join(d, "stream.vpccgof")
    try:
        container.write_container(path, gofs)
        dec = recon.Decoder(path, devices=devices, verify=verify)
        dec.start()
        got = [(fr["n"], _crc(fr["xyz"], fr["rgb"]), fr["digest"], digest_ref.digest_points(fr["xyz"], fr["rgb"])) for fr in dec]
        err = dec.error()
        assert dec.recv_frame() is None
        stats = dec.verify_stats()
        dec.close()
        return got, err, stats
    finally:
        if os.path.exists(path):
            os.remove(path)
        os.rmdir(d)


@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_clean_stream_passes_every_check(monkeypatch, longdress32, devices):
    monkeypatch.delenv("VPCC_DECODER_TEST_CORRUPT", raising=False)
    frames, ref = longdress32
    gofs = [frames[:16], frames[16:]] if devices == (0,) else [frames[:8], frames[8:20], frames[20:]]
    got, err, st = _stream(gofs, devices)
    assert err == ""
    assert [(n, c) for n, c, _, _ in got] == ref
    assert all(dg == want for _, _, dg, want in got)
    assert st["flags"] == 7
    assert st["ingest_frames"] == st["reconstruct_frames"] == st["delivery_frames"] == 32
    assert st["kernel_seconds"] > 0 and st["host_seconds"] > 0


@pytest.mark.parametrize("stage", ["ingest", "reconstruct", "delivery"])
def test_each_stage_is_caught(monkeypatch, longdress32, stage):
    frames, ref = longdress32
    bad = 21                                                # in the second unit, on the second lane
    monkeypatch.setenv("VPCC_DECODER_TEST_CORRUPT", f"{stage}:{bad}")
    got, err, st = _stream([frames[:16], frames[16:]], devices=(0, 0))
    assert f"verify: {stage} mismatch at frame {bad} (expected 0x" in err, err
    assert len(got) == bad                                  # nothing at or after the bad frame
    assert [(n, c) for n, c, _, _ in got] == ref[:bad]


def test_the_hook_corrupts_without_verification(monkeypatch, longdress32):
    monkeypatch.delenv("VPCC_DECODER_VERIFY", raising=False)
    frames, ref = longdress32
    bad = 5
    monkeypatch.setenv("VPCC_DECODER_TEST_CORRUPT", f"reconstruct:{bad}")
    got, err, st = _stream([frames[:16], frames[16:]], verify=None)
    assert err == "" and st["flags"] == 0
    assert len(got) == 32
    assert got[bad][2] is None                              # no digest without the delivery check
    wrong = [i for i in range(32) if (got[i][0], got[i][1]) != ref[i]]
    assert wrong == [bad]


def test_frame_digest_needs_the_delivery_check(monkeypatch, longdress32):
    monkeypatch.delenv("VPCC_DECODER_TEST_CORRUPT", raising=False)
    frames, ref = longdress32
    got, err, st = _stream([frames[:4]], verify="ingest,reconstruct")
    assert err == "" and [(n, c) for n, c, _, _ in got] == ref[:4]
    assert all(dg is None for _, _, dg, _ in got)
    assert st["flags"] == 3 and st["ingest_frames"] == st["reconstruct_frames"] == 4 and st["delivery_frames"] == 0
