"""Cross-modal retrieval over a device-resident gallery of embeddings.

The LvT models end in `similarities = video_emb @ text_emb.T` and an argmax over it.  For a batch that is
`_native.op_similarity`; for a gallery of clips it is a search, and `EmbeddingIndex` is that search: embeddings are
appended to one device buffer, and `search` returns each query's k best rows through the library's fused
score-and-select kernels (`vp_op_topk`: the gallery is read once per group of queries and the [N, Q] score matrix is
never formed).  The search is exact and deterministic: score descending, equal scores by ascending id, and a score
depends on the two vectors alone, so an index sharded over GPUs returns the bits of an unsharded one.

Rows leave with `remove` (tombstones; `compact` drops them for good) and a search takes `allow`, a subset of the rows
per call or per query.  Both are one packed bit per row that the scan consults before a row may enter a list
(`vp_op_topk_masked`), so the result is exactly the search of a gallery that holds the allowed rows alone.

`EmbeddingIndex(dim, dtype=torch.float8_e4m3fn)` stores a row as e4m3 codes and one power-of-two scale, half the
bytes of bfloat16 (`vp_op_quantize_rows_f8`, `vp_op_topk*_f8`); everything above holds for it unchanged, over the
stored values.
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
    """A growing [len, dim] gallery on one GPU, stored in `dtype` (bfloat16, float32 or float8_e4m3fn), and its exact
    top-k search.

    The index does not normalise: scores are plain dot products of what was added.  The LvT models return
    L2-normalised embeddings with `normalize=True` (their default), so indexing and querying with those gives cosine
    similarity.  With a bfloat16 gallery the stored rows are rounded once, in `add`; the queries stay fp32 in effect
    (the kernel carries each as two bf16 terms), so the storage rounding, about 2e-4 in score on unit vectors, is the
    only quantisation.  `dim` must be a multiple of 64 up to 1536; k up to 128.

    `dtype=torch.float8_e4m3fn` is the opt-in small format: a row is `dim` OCP e4m3 codes and one fp32 scale, a power
    of two chosen so that the row's largest magnitude lands in (224, 448], and stands for `codes * scale`: dim + 4
    bytes a row (772 B at dim 768 against bfloat16's 1536 B), so a card holds twice the rows and a search reads half
    the bytes.  `add` quantises on the device straight into the buffers (no full-precision copy of the gallery
    exists); `index.codes` and `index.scales` are views of them and `index.embeddings` is a bfloat16 *copy* of the
    stored values, which is exact (three mantissa bits times a power of two).  Search, groups, `allow`, `remove`,
    `compact` and `comm` work as above and the search is just as exact and deterministic over the stored values; what
    the storage rounding costs is a score error of about 4e-3 max / 1e-3 rms on unit vectors at dim 768 (1.6e-2 / 3e-3
    at dim 64; bfloat16: 3e-4 max) and a recall@10 against the exact search of about 0.95 on unstructured random
    vectors, the hard case.  A row that holds a NaN or an infinity keeps a NaN code there, scores NaN and is never
    returned (a bfloat16 index can return a row that scores +inf).
    """

    def __init__(self, dim: int, dtype=None, device="cuda", capacity: int = 0):
        import torch
        dtype = torch.bfloat16 if dtype is None else dtype
        if dtype not in (torch.bfloat16, torch.float32, torch.float8_e4m3fn):
            raise TypeError(f"dtype must be torch.bfloat16, torch.float32 or torch.float8_e4m3fn, got {dtype}")
        if dim < 64 or dim % 64 or dim > 1536:
            raise NotImplementedError(f"dim must be a multiple of 64 up to 1536, got {dim}")
        self.dim = int(dim)
        self.dtype = dtype
        self.device = torch.device(device)
        self._buf = torch.empty((max(int(capacity), 0), self.dim), dtype=dtype, device=self.device)
        # fp8: the rows' scales, fp32 [capacity]; grown and compacted with the codes in _buf
        self._f8 = dtype == torch.float8_e4m3fn
        self._scales = torch.empty((self.capacity,), dtype=torch.float32, device=self.device) if self._f8 else None
        self._labels = None  # int64 [capacity] once rows are added with `group`
        self._len = 0
        self._alive = None   # uint8 [capacity] once a row was removed: 0 = removed; rows at and past len are 1
        self._removed = 0
        self._live_words = None  # the packed mask of _alive[:len], made when a search needs it

    def __len__(self) -> int:
        return self._len

    @property
    def live(self) -> int:
        """The rows not removed: len(index) minus the tombstones."""
        return self._len - self._removed

    @property
    def capacity(self) -> int:
        return int(self._buf.shape[0])

    @property
    def embeddings(self):
        """The stored [len, dim] rows: a view of the buffer, or on an fp8 index a bfloat16 copy of the values the
        rows stand for (codes * scale, exact in bfloat16)."""
        import torch
        if self._f8:
            return (self.codes.to(torch.float32) * self.scales[:, None]).to(torch.bfloat16)
        return self._buf[:self._len]

    @property
    def codes(self):
        """The stored e4m3 codes, float8_e4m3fn [len, dim] (a view of the buffer); fp8 index only."""
        if not self._f8:
            raise AttributeError("codes: not an fp8 index")
        return self._buf[:self._len]

    @property
    def scales(self):
        """The stored rows' scales, fp32 [len], powers of two (a view of the buffer); fp8 index only."""
        if not self._f8:
            raise AttributeError("scales: not an fp8 index")
        return self._scales[:self._len]

    @property
    def groups(self):
        """The stored rows' labels, int64 [len] (a view of the label buffer); None on an index without labels."""
        return None if self._labels is None else self._labels[:self._len]

    def add(self, emb, group=None) -> range:
        """Appends emb [n, dim] (NumPy or torch, fp32 or bf16), rounded to the storage dtype once; returns the new
        rows' ids, range(len_before, len_after).  The buffer grows by doubling (fp8: codes and scales together).

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
            self._bytes(buf)[:self._len].copy_(self._bytes(self._buf)[:self._len])
            self._buf = buf
            if self._f8:
                scales = torch.empty((cap,), dtype=torch.float32, device=self.device)
                scales[:self._len].copy_(self._scales[:self._len])
                self._scales = scales
            if self._alive is not None:
                alive = torch.ones((cap,), dtype=torch.uint8, device=self.device)
                alive[:self._len].copy_(self._alive[:self._len])
                self._alive = alive
        self._live_words = None
        if labels is not None:
            if self._labels is None or self._labels.shape[0] < self.capacity:  # grows with the rows
                lab = torch.empty((self.capacity,), dtype=torch.int64, device=self.device)
                if self._labels is not None:
                    lab[:self._len].copy_(self._labels[:self._len])
                self._labels = lab
            self._labels[self._len:need].copy_(labels)
        if self._f8:
            if n:
                if emb.stride(1) != 1 or emb.data_ptr() % 16 or (n > 1 and emb.stride(0) * emb.element_size() % 16):
                    emb = emb.contiguous()  # the new rows only
                _native.op_quantize_rows_f8(emb, codes=self._buf[self._len:need], scales=self._scales[self._len:need])
        else:
            self._buf[self._len:need].copy_(emb)
        ids = range(self._len, need)
        self._len = need
        return ids

    def remove(self, ids) -> None:
        """Marks rows as removed: every later search leaves them out, exactly, and a removed row never stands for its
        group.  `ids` are row numbers (an int, or ints in a sequence, NumPy array or tensor); they stay what they
        are, `add` keeps appending and `len(index)` does not change (`live` does).  Removing a row twice is
        harmless; an id outside [0, len) raises ValueError and removes nothing."""
        import torch
        if isinstance(ids, torch.Tensor):
            ids = ids.detach().cpu().numpy()
        rows = np.atleast_1d(np.asarray(ids))
        if rows.ndim != 1 or (rows.size and rows.dtype.kind not in "iu"):
            raise ValueError(f"ids must be integers [n], got {rows.dtype} {tuple(rows.shape)}")
        rows = rows.astype(np.int64)
        if rows.size and (rows.min() < 0 or rows.max() >= self._len):
            bad = rows[(rows < 0) | (rows >= self._len)][0]
            raise ValueError(f"id {int(bad)} is out of range: the index holds rows 0 .. {self._len - 1}")
        if not rows.size:
            return
        if self._alive is None:
            self._alive = torch.ones((self.capacity,), dtype=torch.uint8, device=self.device)
        self._alive[torch.from_numpy(np.unique(rows)).to(self.device)] = 0
        self._removed = self._len - int(self._alive[:self._len].sum())
        self._live_words = None

    def compact(self):
        """Drops the removed rows, and their labels, for good: the survivors move up in order and get new ids
        0 .. live - 1.  Returns old_ids, int64 [new len]: the id each surviving row had.  Afterwards the index has
        no tombstones."""
        import torch
        if self._alive is None or self._removed == 0:
            old_ids = torch.arange(self._len, dtype=torch.int64, device=self.device)
        else:
            old_ids = self._alive[:self._len].nonzero().reshape(-1)
            n = int(old_ids.shape[0])
            buf = self._bytes(self._buf)
            buf[:n] = buf[old_ids]  # the gather is a new tensor, so the rows do not overlap their source
            if self._f8:
                self._scales[:n] = self._scales[old_ids]
            if self._labels is not None:
                self._labels[:n] = self._labels[old_ids]
            self._len = n
        self._alive, self._removed, self._live_words = None, 0, None
        return old_ids

    def _bytes(self, buf):
        """fp8 codes as the bytes they are, for torch's copies and gathers; the other dtypes as they are."""
        import torch
        return buf.view(torch.uint8) if self._f8 else buf

    def _mask(self, allow, Q):
        """The packed mask of a search, int32 [words] or [Q, words], or None when every row is allowed: the
        tombstones, `allow`, or the two ANDed by the pack kernel."""
        import torch
        live = None
        if self._removed:
            if self._live_words is None:
                self._live_words = _native.op_rowmask_pack(self._alive[:self._len])
            live = self._live_words
        if allow is None:
            return live
        if isinstance(allow, np.ndarray):
            if allow.dtype not in (np.bool_, np.uint8):
                raise TypeError(f"allow must be bool or uint8, got {allow.dtype}")
            allow = torch.from_numpy(np.ascontiguousarray(allow))
        if not isinstance(allow, torch.Tensor):
            raise TypeError(f"allow must be a NumPy array or a tensor, got {type(allow).__name__}")
        if allow.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"allow must be bool or uint8, got {allow.dtype}")
        if tuple(allow.shape) not in ((self._len,), (Q, self._len)):
            raise ValueError(f"allow must be [{self._len}] or [{Q}, {self._len}], got {tuple(allow.shape)}")
        return _native.op_rowmask_pack(allow.to(self.device), and_words=live)

    def search(self, queries, k: int, comm=None, id_base: int = 0, allow=None):
        """(scores [Q, k] fp32, ids [Q, k] int64) of queries [Q, dim]: each query's k largest dot products over the
        gallery, score descending and equal scores by ascending id; ids are id_base + row, and with fewer than k
        rows the tail is (-inf, -1).  NumPy in gives NumPy out, tensors in give tensors out.

        `allow` restricts the search to a subset of the rows: bool or uint8 (nonzero = allowed), NumPy or torch,
        [len] for all queries or [Q, len] for a subset per query.  Removed rows are left out whatever it says.  The
        result is the best k of the allowed rows, exactly, with the scores an unrestricted search gives them; rows
        that are not allowed cost little where 64 in a row are not.

        With `comm` (a `distributed.Communicator`) every rank holds a shard: each searches its own rows with its
        `id_base` (the caller's global id of its first row), the [Q, k] lists are gathered over RCCL and every rank
        merges them, so all ranks return the result of searching the whole gallery, bit for bit.  Each rank passes
        its own shard's slice of `allow`."""
        import torch
        q, from_numpy = _as_tensor(queries, self.device)
        if q.dim() != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [Q, {self.dim}], got {tuple(q.shape)}")
        q = q.float().contiguous()
        mask = self._mask(allow, int(q.shape[0]))
        if self._f8 and mask is None:
            scores, ids = _native.op_topk_f8(q, self.codes, self.scales, int(k), id_base=int(id_base))
        elif self._f8:
            scores, ids = _native.op_topk_masked_f8(q, self.codes, self.scales, int(k), mask, id_base=int(id_base))
        elif mask is None:
            scores, ids = _native.op_topk(q, self.embeddings, int(k), id_base=int(id_base))
        else:
            scores, ids = _native.op_topk_masked(q, self.embeddings, int(k), mask, id_base=int(id_base))
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

    def search_groups(self, queries, k: int, comm=None, id_base: int = 0, allow=None):
        """(scores [Q, k] fp32, groups [Q, k] int64, ids [Q, k] int64) of queries [Q, dim]: each query's k best groups
        of rows (`add(emb, group=...)`), a group scoring as its best row, with that row's id (id_base + row; of equal
        scores the smallest).  Score descending, equal scores by ascending id; with fewer than k groups the tail is
        (-inf, -1, -1); rows with a negative label, a NaN or a -inf score never count.  Exact for every k up to 128
        however many rows a group holds: the selection happens in the search kernel's lists (`vp_op_topk_groups`).
        For a gallery of sliding windows, `groups` are the videos and `ids` minus a video's first id is the window.
        NumPy in gives NumPy out, tensors in give tensors out; ValueError on an index without labels.  `allow` as in
        `search`: a row that is removed or not allowed never stands for its group.

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
        mask = self._mask(allow, int(q.shape[0]))
        if self._f8 and mask is None:
            scores, groups, ids = _native.op_topk_groups_f8(q, self.codes, self.scales, self.groups, k,
                                                            id_base=int(id_base))
        elif self._f8:
            scores, groups, ids = _native.op_topk_groups_masked_f8(q, self.codes, self.scales, self.groups, k, mask,
                                                                   id_base=int(id_base))
        elif mask is None:
            scores, groups, ids = _native.op_topk_groups(q, self.embeddings, self.groups, k, id_base=int(id_base))
        else:
            scores, groups, ids = _native.op_topk_groups_masked(q, self.embeddings, self.groups, k, mask,
                                                                id_base=int(id_base))
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
