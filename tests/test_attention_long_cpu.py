"""CPU side of the long-sequence attention work: the streamed kernels'
build-time resources (csrc/attn/attention_long.hip: zero scratch, LDS within
80 KB so two workgroups share a CU), the position-embedding resize, the
weights-only checkpoint load, and the trainer's --image-size / --init-from."""
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None,
                    reason="needs hipcc and c++filt")
def test_long_attention_kernel_resources():
    from tools.kernel_resources import resources
    src = os.path.join(ROOT, "csrc", "attn", "attention_long.hip")
    assert os.path.exists(src), "no long-sequence attention source"
    ks = resources(src)
    names = [k["name"] for k in ks]
    assert any("fwd" in n for n in names), names
    assert any("bwd" in n for n in names), names
    bad = [(k["name"], k["scratch"], k["lds"]) for k in ks if k["scratch"] != "0" or int(k["lds"]) > 81920]
    assert not bad, f"long attention kernels with scratch or more than 80 KB of LDS: {bad}"


def test_resize_pos_embedding():
    from distributed_model_parallel_amd.models.vit import resize_pos_embedding
    torch.manual_seed(0)
    d = 8
    pos = torch.randn(1, 1 + 14 * 14, d)
    assert resize_pos_embedding(pos, 197) is pos  # identity at equal size
    out = resize_pos_embedding(pos, 1 + 24 * 24)
    assert out.shape == (1, 577, d) and out.dtype == pos.dtype
    assert torch.equal(out[:, 0], pos[:, 0])  # class row untouched
    ref = F.interpolate(pos[:, 1:].reshape(1, 14, 14, d).permute(0, 3, 1, 2), size=(24, 24), mode="bicubic",
                        align_corners=False).permute(0, 2, 3, 1).reshape(1, 576, d)
    torch.testing.assert_close(out[:, 1:], ref, atol=0, rtol=0)
    # a constant grid stays constant (bicubic weights sum to 1), the class row keeps its own value
    const = torch.full((1, 197, d), 0.75)
    const[:, 0] = -2.0
    oc = resize_pos_embedding(const, 577)
    torch.testing.assert_close(oc[:, 1:], torch.full((1, 576, d), 0.75), atol=1e-6, rtol=0)
    assert torch.equal(oc[:, 0], const[:, 0])
    # bf16 storage: interpolated in fp32, cast back, class row bit-identical
    pb = pos.bfloat16()
    ob = resize_pos_embedding(pb, 577)
    assert ob.dtype == torch.bfloat16 and ob.shape == (1, 577, d)
    assert torch.equal(ob[:, 0], pb[:, 0])
    refb = F.interpolate(pb[:, 1:].float().reshape(1, 14, 14, d).permute(0, 3, 1, 2), size=(24, 24),
                         mode="bicubic", align_corners=False).permute(0, 2, 3, 1).reshape(1, 576, d).bfloat16()
    assert torch.equal(ob[:, 1:], refb)
    # shrinking works too; a token count that is no square grid + 1 is an error
    assert resize_pos_embedding(pos, 1 + 7 * 7).shape == (1, 50, d)
    with pytest.raises(ValueError):
        resize_pos_embedding(pos, 200)


def test_load_weights_resizes_only_pos_embedding(tmp_path):
    from distributed_model_parallel_amd.models import build_model
    from distributed_model_parallel_amd.models.vit import resize_pos_embedding
    from distributed_model_parallel_amd.utils.checkpoint import load_weights, save_checkpoint
    torch.manual_seed(0)
    src = build_model("vit_tiny", num_classes=10, image_size=32)
    torch.nn.init.normal_(src.head.weight, std=0.1)  # the head is zero-initialised: make the copy visible
    opt = torch.optim.SGD(src.parameters(), lr=0.1, momentum=0.9)
    path = str(tmp_path / "src.pth")
    save_checkpoint(path, src, opt, epoch=7, best_acc=12.5)
    torch.manual_seed(1)
    dst = build_model("vit_tiny", num_classes=10, image_size=48)
    assert dst.pos_embedding.shape == (1, 37, 32)
    rng = torch.get_rng_state()
    info = load_weights(path, dst)
    assert info["pos_embedding_resized"]
    assert torch.equal(torch.get_rng_state(), rng), "load_weights must not restore RNG state"
    want, got = src.state_dict(), dst.state_dict()
    assert want.keys() == got.keys()
    for k in want:
        if k == "pos_embedding":
            assert torch.equal(got[k], resize_pos_embedding(want[k], 37))
            assert torch.equal(got[k][:, 0], want[k][:, 0])
        else:
            assert torch.equal(got[k], want[k]), k
    # same resolution: plain copy
    same = build_model("vit_tiny", num_classes=10, image_size=32)
    assert not load_weights(path, same)["pos_embedding_resized"]
    assert torch.equal(same.pos_embedding, src.pos_embedding)
    # any other mismatch raises
    other = build_model("vit_tiny", num_classes=7, image_size=48)
    with pytest.raises(RuntimeError):
        load_weights(path, other)


def _cli(args, tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(31000 + os.getpid() % 1000), PYTHONPATH=ROOT)
    env.pop("RANK", None)
    return subprocess.run([sys.executable, "-m", "distributed_model_parallel_amd.train.cli", *args,
                           "--log-dir", str(tmp_path / "log"), "--checkpoint", str(tmp_path / "ck.pth")],
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def test_cli_image_size_needs_a_vit(tmp_path):
    r = _cli(["--arch", "mobilenetv2", "--image-size", "48", "--synthetic", "--parallel", "none"], tmp_path)
    assert r.returncode != 0
    assert "--image-size is for ViT archs only" in r.stderr, r.stderr[-2000:]


def test_cli_flag_checks(tmp_path, capsys):
    from distributed_model_parallel_amd.train.cli import build_parser, check_args
    p = build_parser()
    a = p.parse_args(["--arch", "vit_tiny", "--image-size", "48"])
    check_args(p, a)
    assert a.image_size == 48 and a.init_from == ""
    assert p.parse_args([]).image_size is None
    ck = tmp_path / "a.pth"
    ck.write_bytes(b"")
    for argv, msg in ((["--arch", "vit_tiny", "--image-size", "44"], "multiple of the patch size 8"),
                      (["--arch", "resnet50", "--image-size", "384"], "ViT archs only"),
                      (["--arch", "vit_tiny", "--init-from", str(tmp_path / "missing.pth")], "no such file"),
                      (["--arch", "vit_tiny", "--init-from", str(ck), "-r", "--checkpoint", str(ck)],
                       "mutually exclusive")):
        with pytest.raises(SystemExit):
            check_args(p, p.parse_args(argv))
        assert msg in capsys.readouterr().err
    # --resume without a checkpoint to resume from starts fresh, so --init-from may go with it
    check_args(p, p.parse_args(["--arch", "vit_tiny", "--init-from", str(ck), "-r", "--checkpoint",
                                str(tmp_path / "none.pth")]))


def test_cli_trains_vit_at_another_image_size(tmp_path):
    from distributed_model_parallel_amd.models import build_model
    from distributed_model_parallel_amd.utils.checkpoint import save_checkpoint
    torch.manual_seed(0)
    init = str(tmp_path / "init.pth")
    save_checkpoint(init, build_model("vit_tiny", num_classes=10, image_size=32))
    r = _cli(["--arch", "vit_tiny", "--image-size", "48", "--synthetic", "--parallel", "none", "--epochs", "1",
              "--steps-per-epoch", "2", "--dtype", "fp32", "-b", "8", "-j", "0", "--lr", "0.01",
              "--warmup-epochs", "0", "--init-from", init], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = (tmp_path / "log" / "none_8.txt").read_text().strip().splitlines()
    assert len(lines) == 1
    rec = dict(f.split(":", 1) for f in lines[0].split("  "))
    assert math.isfinite(float(rec["loss_train"])) and float(rec["loss_train"]) > 0, lines[0]
    # (model and data agree on 48 px: a 32-px model would fail adding its 17-row
    # position embedding to 37 tokens, 32-px data would fail the same way)
    assert math.isfinite(float(rec["loss_val"])), lines[0]
