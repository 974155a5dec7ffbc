"""What the sharded loader sweeps share (``push.push_prototypes``, ``push.push_prototypes_ppnet``, ``global_explain.nearest_clips``):
the batch header, the store in which the winners' records follow the winners, the cross-rank plumbing and the clip index -> file name
map.  Each sweep keeps its own forward and its own update kernel."""
import numpy as np
import torch

from . import _lib

P_MAX = 4096  # pasn_topk_gather: one launch covers at most this many prototypes


class WinnerStore:
    """One slot store per payload kind for the ``k`` running winners of ``P`` prototypes (``pasn_topk_gather``): ``stores[name]`` is
    ``(P, k) + row_shape`` in the payload's dtype, ``specs[name]`` its (row shape, dtype, fill).  The caller owns the winners' ``index``
    (P, k) int64 and ``slot`` (P, k) int32; the push is the k = 1 case (``slot`` all zero)."""

    def __init__(self, P: int, k: int, device):
        self.P, self.k, self.device = int(P), int(k), device
        self.stores, self.specs = {}, {}

    def _create(self, name: str, row_shape, dtype, fill) -> None:
        self.specs[name] = (row_shape, dtype, fill)
        self.stores[name] = torch.full((self.P, self.k) + row_shape, fill, dtype=dtype, device=self.device)

    def gather(self, name: str, payload: torch.Tensor, per_proto: bool, index, slot, index_base: int, fill=0) -> None:
        """``payload`` (B, P, ...) with ``per_proto`` else (B, ...): the rows of the winners that lie in this batch (global index in
        ``[index_base, index_base + B)``) are copied into ``stores[name]``; called after the batch's update of ``index`` / ``slot``."""
        payload = payload.contiguous()
        row_shape = tuple(payload.shape[2 if per_proto else 1:])
        if name not in self.stores:
            self._create(name, row_shape, payload.dtype, fill)
        elif self.specs[name][:2] != (row_shape, payload.dtype):
            raise ValueError(f"payload {name!r}: rows {row_shape} {payload.dtype} do not match the store's {self.specs[name][:2]}")
        _lib.check(_lib.lib().pasn_topk_gather(
            index.data_ptr(), slot.data_ptr(), payload.data_ptr(), self.stores[name].data_ptr(), int(payload.shape[0]), self.P, self.k,
            int(np.prod(row_shape, dtype=np.int64)), payload.element_size(), int(per_proto), int(index_base), _lib.current_stream()))

    def resolved(self, name: str, index, slot) -> torch.Tensor:
        """``stores[name]`` in row order (slot indirection resolved); empty entries (``index < 0``) read the store's fill value."""
        store = self.stores[name]
        rows = store[torch.arange(self.P, device=store.device)[:, None], slot.long()]
        valid = (index >= 0).view((self.P, self.k) + (1,) * (store.dim() - 2))
        return torch.where(valid, rows, store.new_full((), self.specs[name][2]))

    def agree(self, world_size: int) -> bool:
        """After the sweep: a rank whose shard held no batch builds empty stores to the specs of the other ranks'.  False when no
        rank saw a batch."""
        specs = first_across_ranks(self.specs or None) if world_size > 1 else self.specs
        if specs and not self.stores:
            for name, spec in specs.items():  # in the order the other ranks created theirs
                self._create(name, *spec)
        return bool(specs)


def sweep_batches(dataloader, device, rank: int, world_size: int, preprocess_input_function=None):
    """The header of a sweep over this rank's shard (``push._iter_shard``): yields ``(batch number, global index of the batch's first
    clip, sample, the preprocessed input on the device, the int64 labels on the device)``; the label copy is issued first and does not
    stall the host (``push._labels_to_device``)."""
    from .push import _iter_shard, _labels_to_device

    pinned = []
    for i, base, sample in _iter_shard(dataloader, rank, world_size):
        x = sample["cine"]
        if preprocess_input_function is not None:
            x = preprocess_input_function(x)
        labels = _labels_to_device(sample["target_AS"], device, pinned)
        yield i, int(base), sample, x.to(device), labels


def gather_ranks(tensors, device):
    """all_gather of each tensor: per rank, the tuple of that rank's tensors, back on ``device``."""
    import torch.distributed as dist

    from .push import _for_collective

    world = dist.get_world_size()
    gathered = []
    for t in tensors:
        t = _for_collective(t.contiguous())
        buf = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(buf, t)
        gathered.append([b.to(device) for b in buf])
    return [tuple(g[r] for g in gathered) for r in range(world)]


def first_across_ranks(value):
    """The first value, in rank order, that is not None (what a rank with an empty shard has to take from the others), or None."""
    import torch.distributed as dist

    every = [None] * dist.get_world_size()
    dist.all_gather_object(every, value)
    return next((v for v in every if v is not None), None)


def filenames_at(names: dict, index):
    """``names``: {global index of a batch's first clip: the batch's file names}.  The file name of every global clip index in
    ``index`` (any shape) as nested lists of that shape; None for index -1 and for a clip its batch has no name for."""
    idx = torch.as_tensor(index).detach().cpu().numpy().astype(np.int64)
    bases = np.array(sorted(names), dtype=np.int64)
    at = np.searchsorted(bases, idx.reshape(-1), side="right") - 1  # the batch of each index: the last base at or below it
    out = np.empty(idx.size, dtype=object)  # of None
    for n, (g, a) in enumerate(zip(idx.reshape(-1), at)):
        if g >= 0 and a >= 0 and g - bases[a] < len(names[int(bases[a])]):
            out[n] = names[int(bases[a])][g - bases[a]]
    return out.reshape(idx.shape).tolist()
