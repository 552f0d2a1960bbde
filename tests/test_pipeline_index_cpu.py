"""``pipeline._index_to``: how ``PairedBatches`` sends its small index tensors (``order``, ``where``, ``pos``) to the GPU.
(``PairedBatches`` itself requires a GPU -- there is no CPU path of it to test; ``tests/test_gpu_pipeline.py`` covers its
outputs.)  Needs no GPU."""
import torch


def test_index_to_the_current_device_goes_through_the_non_blocking_upload(monkeypatch):
    from myrtlespeech_amd import _lib, pipeline
    sent = []
    monkeypatch.setattr(_lib, "upload", lambda t: sent.append(t) or t)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    both = torch.tensor([5, 9, 9, 2, 7])
    order = torch.sort(both, descending=True, stable=True).indices
    where = torch.empty_like(order)
    where[order] = torch.arange(order.numel())
    for dev in (torch.device("cuda"), torch.device("cuda", 0)):
        for index in (order, where, where[1:4]):                       # (`pos` is a slice of `where`)
            assert pipeline._index_to(index, dev) is index
    assert len(sent) == 6
    # what the pair's cut-back relies on: `where` undoes `order`
    x = torch.arange(5.0)
    assert torch.equal(x.index_select(0, order).index_select(0, where), x)


def test_index_to_another_device_is_a_plain_copy(monkeypatch):
    """``_lib.upload`` targets the current device: an index for inputs on another one must not go through it."""
    from myrtlespeech_amd import _lib, pipeline
    sent = []
    monkeypatch.setattr(_lib, "upload", lambda t: sent.append(t) or t)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    out = None
    try:
        out = pipeline._index_to(torch.tensor([2, 0, 1]), torch.device("cuda", 1))
    except (RuntimeError, AssertionError):                             # no such device here: the copy itself was refused
        pass
    assert not sent
    assert out is None or (out.device == torch.device("cuda", 1) and out.cpu().tolist() == [2, 0, 1])
