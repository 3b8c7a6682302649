"""Cross-modal retrieval over a device-resident gallery of embeddings.

The LvT models end in `similarities = video_emb @ text_emb.T` and an argmax over it.  For a batch that is
`_native.op_similarity`; for a gallery of clips it is a search, and `EmbeddingIndex` is that search: embeddings are
appended to one device buffer, and `search` returns each query's k best rows through the library's fused
score-and-select kernels (`vp_op_topk`: the gallery is read once per group of queries and the [N, Q] score matrix is
never formed).  The search is exact and deterministic: score descending, equal scores by ascending id, and a score
depends on the two vectors alone, so an index sharded over GPUs returns the bits of an unsharded one.
"""

from __future__ import annotations

import numpy as np

from . import _native


def _as_tensor(x, device):
    import torch
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x)).to(device), True
    return x.to(device), False


class EmbeddingIndex:
    """A growing [len, dim] gallery on one GPU, stored in `dtype` (bfloat16 or float32), and its exact top-k search.

    The index does not normalise: scores are plain dot products of what was added.  The LvT models return
    L2-normalised embeddings with `normalize=True` (their default), so indexing and querying with those gives cosine
    similarity.  With a bfloat16 gallery the stored rows are rounded once, in `add`; the queries stay fp32 in effect
    (the kernel carries each as two bf16 terms), so the storage rounding, about 2e-4 in score on unit vectors, is the
    only quantisation.  `dim` must be a multiple of 64 up to 1536; k up to 128.
    """

    def __init__(self, dim: int, dtype=None, device="cuda", capacity: int = 0):
        import torch
        dtype = torch.bfloat16 if dtype is None else dtype
        if dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"dtype must be torch.bfloat16 or torch.float32, got {dtype}")
        if dim < 64 or dim % 64 or dim > 1536:
            raise NotImplementedError(f"dim must be a multiple of 64 up to 1536, got {dim}")
        self.dim = int(dim)
        self.dtype = dtype
        self.device = torch.device(device)
        self._buf = torch.empty((max(int(capacity), 0), self.dim), dtype=dtype, device=self.device)
        self._labels = None  # int64 [capacity] once rows are added with `group`
        self._len = 0

    def __len__(self) -> int:
        return self._len

    @property
    def capacity(self) -> int:
        return int(self._buf.shape[0])

    @property
    def embeddings(self):
        """The stored [len, dim] rows (a view of the buffer)."""
        return self._buf[:self._len]

    @property
    def groups(self):
        """The stored rows' labels, int64 [len] (a view of the label buffer); None on an index without labels."""
        return None if self._labels is None else self._labels[:self._len]

    def add(self, emb, group=None) -> range:
        """Appends emb [n, dim] (NumPy or torch, fp32 or bf16), rounded to the storage dtype once; returns the new
        rows' ids, range(len_before, len_after).  The buffer grows by doubling.

        `group` labels the new rows for `search_groups`: an int (every new row belongs to that one group, for example
        all windows of one video) or an int64 array [n]; a negative label blanks a row out of the grouped search.  An
        index holds labels for all of its rows or for none: mixing the two kinds of `add` raises ValueError."""
        import torch
        emb, _ = _as_tensor(emb, self.device)
        if emb.dim() != 2 or emb.shape[1] != self.dim:
            raise ValueError(f"emb must be [n, {self.dim}], got {tuple(emb.shape)}")
        if emb.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"emb must be fp32 or bf16, got {emb.dtype}")
        n = int(emb.shape[0])
        if group is None and self._labels is not None:
            raise ValueError("this index holds group labels: add(emb, group=...) is required")
        if group is not None and self._labels is None and self._len > 0:
            raise ValueError("this index holds rows without group labels: add(emb) without group is required")
        labels = None
        if group is not None:
            if isinstance(group, (int, np.integer)):
                labels = torch.full((n,), int(group), dtype=torch.int64, device=self.device)
            else:
                labels, _ = _as_tensor(group, self.device)
                if labels.dtype != torch.int64 or tuple(labels.shape) != (n,):
                    raise ValueError(f"group must be an int or int64 [{n}], got {labels.dtype} {tuple(labels.shape)}")
        need = self._len + n
        if need > self.capacity:
            cap = max(self.capacity, 1)
            while cap < need:
                cap *= 2
            buf = torch.empty((cap, self.dim), dtype=self.dtype, device=self.device)
            buf[:self._len].copy_(self._buf[:self._len])
            self._buf = buf
        if labels is not None:
            if self._labels is None or self._labels.shape[0] < self.capacity:  # grows with the rows
                lab = torch.empty((self.capacity,), dtype=torch.int64, device=self.device)
                if self._labels is not None:
                    lab[:self._len].copy_(self._labels[:self._len])
                self._labels = lab
            self._labels[self._len:need].copy_(labels)
        self._buf[self._len:need].copy_(emb)
        ids = range(self._len, need)
        self._len = need
        return ids

    def search(self, queries, k: int, comm=None, id_base: int = 0):
        """(scores [Q, k] fp32, ids [Q, k] int64) of queries [Q, dim]: each query's k largest dot products over the
        gallery, score descending and equal scores by ascending id; ids are id_base + row, and with fewer than k
        rows the tail is (-inf, -1).  NumPy in gives NumPy out, tensors in give tensors out.

        With `comm` (a `distributed.Communicator`) every rank holds a shard: each searches its own rows with its
        `id_base` (the caller's global id of its first row), the [Q, k] lists are gathered over RCCL and every rank
        merges them, so all ranks return the result of searching the whole gallery, bit for bit."""
        import torch
        q, from_numpy = _as_tensor(queries, self.device)
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [Q, {self.dim}], got {tuple(q.shape)}")
        q = q.float().contiguous()
        scores, ids = _native.op_topk(q, self.embeddings, int(k), id_base=int(id_base))
        if comm is not None and q.shape[0] > 0:
            Q = int(q.shape[0])
            counts = [Q] * comm.world
            all_s = comm.all_gather_rows(scores, counts=counts)
            # int64 ids travel as bytes: the gather takes fp32, bf16 and uint8
            all_i = comm.all_gather_rows(ids.view(torch.uint8), counts=counts).view(torch.int64)
            scores, ids = _native.op_topk_merge(all_s.view(comm.world, Q, int(k)), all_i.view(comm.world, Q, int(k)),
                                                int(k))
        if from_numpy:
            return scores.cpu().numpy(), ids.cpu().numpy()
        return scores, ids

    def search_groups(self, queries, k: int, comm=None, id_base: int = 0):
        """(scores [Q, k] fp32, groups [Q, k] int64, ids [Q, k] int64) of queries [Q, dim]: each query's k best groups
        of rows (`add(emb, group=...)`), a group scoring as its best row, with that row's id (id_base + row; of equal
        scores the smallest).  Score descending, equal scores by ascending id; with fewer than k groups the tail is
        (-inf, -1, -1); rows with a negative label, a NaN or a -inf score never count.  Exact for every k up to 128
        however many rows a group holds: the selection happens in the search kernel's lists (`vp_op_topk_groups`).
        For a gallery of sliding windows, `groups` are the videos and `ids` minus a video's first id is the window.
        NumPy in gives NumPy out, tensors in give tensors out; ValueError on an index without labels.

        With `comm` every rank holds a shard (groups may span shards): the three lists are gathered as `search`
        gathers its two and merged on every rank, to the bits of the whole gallery's search."""
        import torch
        if self._labels is None:
            raise ValueError("search_groups needs group labels: add(emb, group=...)")
        q, from_numpy = _as_tensor(queries, self.device)
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [Q, {self.dim}], got {tuple(q.shape)}")
        q = q.float().contiguous()
        k = int(k)
        scores, groups, ids = _native.op_topk_groups(q, self.embeddings, self.groups, k, id_base=int(id_base))
        if comm is not None and q.shape[0] > 0:
            Q = int(q.shape[0])
            counts = [Q] * comm.world
            all_s = comm.all_gather_rows(scores, counts=counts)
            all_g = comm.all_gather_rows(groups.view(torch.uint8), counts=counts).view(torch.int64)
            all_i = comm.all_gather_rows(ids.view(torch.uint8), counts=counts).view(torch.int64)
            scores, groups, ids = _native.op_topk_groups_merge(
                all_s.view(comm.world, Q, k), all_g.view(comm.world, Q, k), all_i.view(comm.world, Q, k), k)
        if from_numpy:
            return scores.cpu().numpy(), groups.cpu().numpy(), ids.cpu().numpy()
        return scores, groups, ids
