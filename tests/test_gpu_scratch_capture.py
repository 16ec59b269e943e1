"""-m gpu: the capture rule of the library's grow-only scratch (pit_hip._lib._Scratch), for every class built on it -- a buffer
is never replaced during or after a HIP graph capture that used it.  No library kernel runs under capture: the graphs record one
fill of a preallocated tensor, and are not replayed."""
import pytest
import torch

from gpu_common import DEV

pytestmark = pytest.mark.gpu


def _cases():
    from pit_hip import _lib

    # name -> (factory, take(ws, device), a request that needs a bigger / another buffer, one that fits the same buffer)
    return {
        "workspace": (_lib.Workspace, lambda w, d: w.get(64, 1024, 16, d), lambda w, d: w.get(65536, 65536, 16, d),
                      lambda w, d: w.get(8, 1024, 16, d)),
        # the cache belongs to ONE codebook shape: any other shape would have to replace it
        "cache": (_lib.Workspace, lambda w, d: w.cache(1024, 16, d), lambda w, d: w.cache(4096, 16, d),
                  lambda w, d: w.cache(1024, 16, d)),
        "vq_backward": (_lib.VqBackwardWorkspace, lambda w, d: w.get(64, 1024, 16, d), lambda w, d: w.get(65536, 65536, 16, d),
                        lambda w, d: w.get(8, 1024, 16, d)),
        "lfq_train": (_lib.LfqTrainWorkspace, lambda w, d: w.get(64, 8, d), lambda w, d: w.get(65536, 16, d),
                      lambda w, d: w.get(8, 8, d)),
    }


@pytest.mark.parametrize("name", ["workspace", "cache", "vq_backward", "lfq_train"])
def test_scratch_is_never_replaced_during_or_after_a_capture(name):
    from pit_hip import _lib

    make, take, bigger, smaller = _cases()[name]
    dev = torch.zeros(1, device=DEV).device
    t = torch.zeros(16, device=dev)

    ws = make()                                        # fresh: a capture would have to allocate
    with pytest.raises(_lib.GqHipError, match="warm-up"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            t.fill_(1.0)
            take(ws, dev)

    ws = make()
    ptr, nbytes = take(ws, dev)                        # the eager warm-up
    assert ptr and nbytes > 0
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        t.fill_(1.0)
        assert take(ws, dev) == (ptr, nbytes)
    with pytest.raises(_lib.GqHipError, match="warm-up"):
        bigger(ws, dev)
    assert smaller(ws, dev) == (ptr, nbytes)
    torch.cuda.synchronize()


def test_a_codebook_shape_without_a_cache_has_nothing_to_pin():
    """(1024, 4) keeps no codebook cache (gqhip_cb_cache_bytes is 0): ``cache`` answers (None, 0) in and out of a capture, allocates
    nothing, and leaves the workspace free to grow."""
    from pit_hip import _lib

    dev = torch.zeros(1, device=DEV).device
    t = torch.zeros(16, device=dev)
    assert _lib.lib().gqhip_cb_cache_bytes(1024, 4) == 0
    ws = _lib.Workspace()
    assert ws.cache(1024, 4, dev) == (None, 0)
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        t.fill_(1.0)
        assert ws.cache(1024, 4, dev) == (None, 0)
    assert ws.cache_buf is None
    ptr, nbytes = ws.get(64, 1024, 16, dev)
    assert ptr and nbytes > 0
    torch.cuda.synchronize()


def test_workspace_keeps_one_pin_for_scratch_and_cache():
    """A capture that used the scratch also pins the codebook cache, and the other way round."""
    from pit_hip import _lib

    dev = torch.zeros(1, device=DEV).device
    t = torch.zeros(16, device=dev)
    for first, other in ((lambda w: w.get(64, 1024, 16, dev), lambda w: w.cache(1024, 16, dev)),
                         (lambda w: w.cache(1024, 16, dev), lambda w: w.get(64, 1024, 16, dev))):
        ws = _lib.Workspace()
        first(ws)
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            t.fill_(1.0)
            first(ws)
        with pytest.raises(_lib.GqHipError, match="warm-up"):
            other(ws)
    torch.cuda.synchronize()
