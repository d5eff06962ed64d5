"""tfevents writer + config decoder + param snapshot tests."""

import json
import os
import struct

import torch

from distributed_sac_amd.config import Decoder, cfg_read
from distributed_sac_amd.utils.tfevents import (TFEventWriter, _crc32c,
                                                _masked_crc)
from distributed_sac_amd.workers.param_server import ParamSnapshot


def test_crc32c_known_vectors():
    # standard CRC32C test vector
    assert _crc32c(b"123456789") == 0xE3069283
    assert _crc32c(b"") == 0


def test_tfevents_roundtrip(tmp_path):
    w = TFEventWriter(str(tmp_path))
    w.add_scalar("loss", 1.5, 10)
    w.add_scalar("loss", 0.5, 20)
    w.close()
    files = os.listdir(tmp_path)
    assert len(files) == 1
    data = open(os.path.join(tmp_path, files[0]), "rb").read()
    # walk records verifying framing + CRCs
    off, n = 0, 0
    while off < len(data):
        (length,) = struct.unpack("<Q", data[off:off + 8])
        (hcrc,) = struct.unpack("<I", data[off + 8:off + 12])
        assert hcrc == _masked_crc(data[off:off + 8])
        payload = data[off + 12:off + 12 + length]
        (dcrc,) = struct.unpack("<I", data[off + 12 + length:off + 16 + length])
        assert dcrc == _masked_crc(payload)
        off += 16 + length
        n += 1
    assert n == 3  # file_version + 2 scalars
    assert b"loss" in data
    assert b"brain.Event:2" in data


def test_config_decoder_string_int_coercion(tmp_path):
    """Reference Decoder coerces numeric strings to int (utils.py:4-20)."""
    raw = {"a": "5", "b": {"c": "10", "d": "hello"}, "e": [1.5, "7"],
           "f": 1e6, "g": 3e-4}
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(raw))
    cfg = cfg_read(str(p))
    assert cfg["a"] == 5 and isinstance(cfg["a"], int)
    assert cfg["b"]["c"] == 10
    assert cfg["b"]["d"] == "hello"
    assert cfg["e"] == [1.5, 7]
    assert cfg["f"] == 1e6 and isinstance(cfg["f"], float)
    assert cfg["g"] == 3e-4


def test_param_snapshot_seqlock():
    snap = ParamSnapshot(16)
    src = torch.arange(16, dtype=torch.float32)
    out = torch.zeros(16)
    assert snap.read(out, last_iteration=0) is None  # nothing published
    snap.publish(src, iteration=3)
    it = snap.read(out, last_iteration=0)
    assert it == 3
    assert torch.equal(out, src)
    # unchanged iteration -> no copy
    assert snap.read(out, last_iteration=3) is None
    snap.publish(src * 2, iteration=9)
    it = snap.read(out, last_iteration=3)
    assert it == 9 and torch.equal(out, src * 2)


def test_cfg_value_parity_with_reference():
    """Our regenerated cfg JSONs must carry the same hyperparameter VALUES
    as the reference's shipped cfgs (parsed with the same string-coercion
    Decoder) — the reference's checkpoints and training behavior depend on
    them.  Compares recursively; our files may ADD keys (e.g. the CARE
    encoder block records RoBERTa_embedding_dim explicitly) but may not
    change or drop any reference key."""
    import json

    from distributed_sac_amd.config import Decoder

    # the reference's shipped cfgs, stored verbatim as fixtures
    ref_root = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                            "golden", "reference_cfg")
    here = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "cfg")

    def load(p):
        with open(p) as f:
            return json.load(f, cls=Decoder)

    def check(ours, ref, path=""):
        for k, rv in ref.items():
            assert k in ours, f"missing reference cfg key {path}{k}"
            ov = ours[k]
            if isinstance(rv, dict):
                check(ov, rv, f"{path}{k}.")
            elif k.endswith("_json_path"):
                # metadata paths are repo-relative in both trees; compare
                # the file NAME (layout differs by design)
                assert os.path.basename(str(ov)) == os.path.basename(str(rv)), \
                    f"{path}{k}: {ov!r} vs {rv!r}"
            else:
                assert ov == rv, f"{path}{k}: ours={ov!r} ref={rv!r}"

    names = [
        "LunarLanderContinuous-v2_Distributed_SAC_cfg.json",
        "MT1_Distributed_VSAC_cfg.json",
        "MT1_Distributed_CARE_cfg.json",
        "MT10_Distributed_MTSAC_cfg.json",
        "MT10_Distributed_CARE_cfg.json",
    ]
    for n in names:
        check(load(os.path.join(here, n)),
              load(os.path.join(ref_root, n)))


def test_tfevents_reader_roundtrip(tmp_path):
    """Writer -> reader roundtrip: scalars come back tag/step/value-exact
    (the reader hand-decodes the protobuf; no tensorboard installed)."""
    from distributed_sac_amd.analysis.read_tfevents import read_scalars_dir

    w = TFEventWriter(str(tmp_path))
    w.add_scalar("a/loss", 1.25, 3)
    w.add_scalar("a/loss", 0.75, 7)
    w.add_scalar("b/rate", 42.0, 1)
    w.close()
    series = read_scalars_dir(str(tmp_path))
    assert series["a/loss"] == [(3, 1.25), (7, 0.75)]
    assert series["b/rate"] == [(1, 42.0)]
