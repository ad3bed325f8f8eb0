"""CPU: the host side of merlin_group_clip_sgd / merlin_episode_loss (include/merlin_hip.h): workspace sizes, the
no-op cases and the argument checks, none of which queues device work."""
import ctypes as C


def test_group_clip_sgd_host_checks():
    from merlin import _native as nat

    L = nat.lib()
    numel = (C.c_int64 * 3)(10, 4096, 5000)
    assert L.merlin_group_clip_sgd_workspace(3, numel, 4) == (1 + 4 + 5) * 4  # 1024-element blocks per task x G
    assert L.merlin_group_clip_sgd_workspace(3, numel, 0) == 1
    assert L.merlin_group_clip_sgd_workspace(33, numel, 4) == -1
    assert L.merlin_group_clip_sgd_workspace(3, (C.c_int64 * 3)(10, 0, 5), 4) == -1
    # G = 0 or no tensors: success without a launch
    assert L.merlin_group_clip_sgd(0, None, None, None, 4, 0.01, 0.5, None, None, None) == 0
    assert L.merlin_group_clip_sgd(3, None, None, numel, 0, 0.01, 0.5, None, None, None) == 0
    assert L.merlin_group_clip_sgd(33, None, None, numel, 4, 0.01, 0.5, None, None, None) == 1
    assert L.merlin_group_clip_sgd(3, None, None, numel, 4, 0.01, 0.5, None, None, None) == 1  # null lists
    nul = (C.c_void_p * 3)()
    ws = (C.c_double * 40)()
    assert L.merlin_group_clip_sgd(3, nul, nul, numel, 4, 0.01, 0.5, None, ws, None) == 1  # null tensor pointers
    assert b"null" in L.merlin_last_error()
    assert L.merlin_group_clip_sgd(3, nul, nul, numel, 1 << 20, 0.01, 0.5, None, ws, None) == 1  # G over the grid limit


def test_episode_loss_host_checks():
    from merlin import _native as nat

    L = nat.lib()
    assert L.merlin_episode_loss(None, None, None, None, None, 9, 0, 0.995, 0.95, None, None, None) == 0  # no episodes
    assert L.merlin_episode_loss(None, None, None, None, None, 0, 5, 0.995, 0.95, None, None, None) == 1
    assert L.merlin_episode_loss(None, None, None, None, None, 9, 5, 0.995, 0.95, None, None, None) == 1
    assert b"null" in L.merlin_last_error()


def test_few_shot_is_exported():
    import merlin
    from merlin.evaluation import evaluate_few_shot  # noqa: F401

    assert "FewShotAdapter" in merlin.__all__ and merlin.FewShotAdapter.__module__ == "merlin.few_shot"
