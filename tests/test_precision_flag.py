"""--gemm_precision through the CLI, the config dataclass and the agent
constructor (no GPU): the default is fp32, bf16 is accepted by the parser and
carried by D4PGConfig, and the eager backend refuses it."""

import pytest

from d4pg_amd.config import D4PGConfig, make_parser


def test_parser_default_is_fp32():
    args = make_parser().parse_args([])
    assert args.gemm_precision == "fp32"
    assert D4PGConfig().gemm_precision == "fp32"


def test_parser_accepts_bf16_and_rejects_others():
    args = make_parser().parse_args(["--gemm_precision", "bf16"])
    assert args.gemm_precision == "bf16"
    with pytest.raises(SystemExit):
        make_parser().parse_args(["--gemm_precision", "fp16"])


def test_config_from_args_carries_the_field():
    args = make_parser().parse_args(["--gemm_precision", "bf16",
                                     "--bsize", "1024"])
    cfg = D4PGConfig.from_args(args)
    assert cfg.gemm_precision == "bf16"
    assert "gemm_precision" not in cfg.extra


def test_eager_backend_refuses_bf16():
    from d4pg_amd.algo.d4pg import DDPG
    with pytest.raises(ValueError, match="gemm_precision"):
        DDPG(3, 1, backend="eager", gemm_precision="bf16")
    with pytest.raises(ValueError, match="gemm_precision"):
        DDPG(3, 1, backend="eager", gemm_precision="tf32")
    assert DDPG(3, 1, backend="eager").gemm_precision == "fp32"


def test_train_cli_passes_the_flag_to_the_agent(monkeypatch):
    """train.main builds its agent with --gemm_precision."""
    import train

    class Built(Exception):
        pass

    def fake_ddpg(*a, **kw):
        raise Built(kw.get("gemm_precision"))

    monkeypatch.setattr(train, "DDPG", fake_ddpg)
    for argv, want in ((["--gemm_precision", "bf16"], "bf16"), ([], "fp32")):
        with pytest.raises(Built) as e:
            train.main(["--device", "cpu", "--backend", "eager"] + argv)
        assert e.value.args[0] == want


def test_train_cli_eager_refuses_bf16():
    import train
    with pytest.raises(ValueError, match="gemm_precision"):
        train.main(["--device", "cpu", "--backend", "eager",
                    "--gemm_precision", "bf16"])
