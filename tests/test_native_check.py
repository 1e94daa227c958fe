"""``mdtf.ops._native.check``: the status check after every native launch and its ``MDTF_SYNC_CHECK=1`` debug mode
(synchronize after each launch, so a faulting kernel is named).  CPU only: the torch.cuda calls are stubbed."""
import pytest
import torch

from mdtf.ops import _native

MDTF_EINVAL = -1


@pytest.fixture
def sync_check(monkeypatch):
    calls = {"sync": 0, "capturing": False, "error": None, "initialized": True}

    def synchronize(*a, **k):
        calls["sync"] += 1
        if calls["error"] is not None:
            raise RuntimeError(calls["error"])

    monkeypatch.setattr(torch.cuda, "is_initialized", lambda: calls["initialized"])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: calls["capturing"])
    monkeypatch.setattr(torch.cuda, "synchronize", synchronize)
    monkeypatch.setattr(_native, "_SYNC_CHECK", True)
    return calls


def test_sync_check_success_returns_none(sync_check):
    assert _native.check(0, "x") is None
    assert sync_check["sync"] == 1


def test_sync_check_names_the_faulting_kernel(sync_check):
    sync_check["error"] = "HIP error: an illegal memory access was encountered"
    with pytest.raises(RuntimeError, match=r"mdtf kernel x faulted: HIP error: an illegal memory access"):
        _native.check(0, "x")
    assert sync_check["sync"] == 1


def test_sync_check_skipped_while_capturing(sync_check):
    sync_check["capturing"] = True
    sync_check["error"] = "synchronize during capture"
    assert _native.check(0, "x") is None
    assert sync_check["sync"] == 0


def test_sync_check_without_a_gpu_context_is_a_no_op(sync_check):
    sync_check["initialized"] = False
    sync_check["error"] = "no device"
    assert _native.check(0, "x") is None
    assert sync_check["sync"] == 0


def test_sync_check_off_does_not_synchronize(sync_check, monkeypatch):
    monkeypatch.setattr(_native, "_SYNC_CHECK", False)
    assert _native.check(0, "x") is None
    assert sync_check["sync"] == 0


@pytest.mark.parametrize("on", [False, True])
def test_failed_status_names_kernel_and_reason(sync_check, monkeypatch, on):
    monkeypatch.setattr(_native, "_SYNC_CHECK", on)
    with pytest.raises(RuntimeError, match=r"mdtf kernel x failed: invalid argument \(code -1\)"):
        _native.check(MDTF_EINVAL, "x")
    assert sync_check["sync"] == 0
