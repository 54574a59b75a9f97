"""CPU-only checks of the "high" fp32 matmul precision (split-bf16 gather GEMM): the C ABI declares and exports the setter,
the models validate the argument before any device work, and both trainers pass their flag through to the model."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_setter_and_the_library_binds_it():
    import rcgan_amd  # noqa: F401
    from rcgan_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rcgan_hip.h")).read()
    assert re.search(r"int rcgan_set_f32_matmul_precision\(rcgan_ctx\* ctx, int precision\);", hdr)
    assert re.search(r"#define RCGAN_F32_PRECISION_HIGHEST 0\b", hdr)
    assert re.search(r"#define RCGAN_F32_PRECISION_HIGH 1\b", hdr)
    assert (_lib.F32_PRECISION_HIGHEST, _lib.F32_PRECISION_HIGH) == (0, 1)
    for half in ("bf16", "f16"):
        fn = _lib.load(half).rcgan_set_f32_matmul_precision
        assert fn.argtypes is not None and len(fn.argtypes) == 2


@pytest.mark.parametrize("kwargs", [dict(dtype="bf16", f32_matmul_precision="high"),
                                    dict(dtype="f16", f32_matmul_precision="high"),
                                    dict(dtype="f32", f32_matmul_precision="fast"),
                                    dict(dtype="f32", f32_matmul_precision="HIGH")])
def test_cifar_model_rejects_a_bad_precision_before_touching_a_device(kwargs):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.cifar import CifarRCGAN
    with pytest.raises(ValueError, match="f32_matmul_precision"):
        CifarRCGAN(batch_size=4, use_graphs=False, **kwargs)


@pytest.mark.parametrize("kwargs", [dict(dtype="f32", f32_matmul_precision="fast"),
                                    dict(dtype="bf16", f32_matmul_precision="high"),
                                    dict(dtype="f32", f32_matmul_precision=None)])
def test_mnist_model_rejects_a_bad_precision_before_touching_a_device(kwargs):
    import rcgan_amd  # noqa: F401
    from rcgan_amd.mnist import MnistRCGAN
    with pytest.raises(ValueError, match="f32_matmul_precision"):
        MnistRCGAN(batch_size=4, use_graphs=False, **kwargs)


class _Built(Exception):
    pass


def _capture(kwargs_out):
    def fake(*args, **kwargs):
        kwargs_out.update(kwargs)
        raise _Built()
    return fake


@pytest.mark.parametrize("flag", [None, "highest", "high"])
def test_cifar_trainer_flag_reaches_the_model(flag, tmp_path, monkeypatch):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import cifar, train_cifar
    assert train_cifar.define_flags().parse([]).f32_matmul_precision == "highest"
    got = {}
    monkeypatch.setattr(cifar, "CifarRCGAN", _capture(got))
    argv = ["--log_file", str(tmp_path / "log.txt"), "--parent_dir", str(tmp_path), "--ngpus", "1", "--dtype", "f32",
            "--synthetic", "--niters", "1"] + ([] if flag is None else ["--f32_matmul_precision", flag])
    with pytest.raises(_Built):
        train_cifar.main(argv)
    assert got["f32_matmul_precision"] == (flag or "highest")
    assert got["dtype"] == "f32"


@pytest.mark.parametrize("flag", [None, "highest", "high"])
def test_mnist_trainer_flag_reaches_the_model(flag, tmp_path, monkeypatch):
    import rcgan_amd  # noqa: F401
    from rcgan_amd import mnist, train_mnist
    assert train_mnist.define_flags().parse([]).f32_matmul_precision == "highest"
    got = {}
    monkeypatch.setattr(mnist, "MnistRCGAN", _capture(got))
    argv = ["--checkpoint_dir", str(tmp_path), "--synthetic", "--synthetic_size", "200", "--epoch", "1"] + \
        ([] if flag is None else ["--f32_matmul_precision", flag])
    with pytest.raises(_Built):
        train_mnist.main(argv)
    assert got["f32_matmul_precision"] == (flag or "highest")
