"""ctypes / torch front of the packed embedding layer (include/word2bits_embed.h).

    emb = PackedEmbedding("vectors.w2bp")                       # the table stays packed on the device: 1 or 2 bits a value
    rows = emb.lookup([3, 17, -1])                              # numpy float32 [3, dim]; id < 0 is padding (a zero row)
    sent = emb.bag(ids, offsets, mode="mean")                   # numpy [n_bags, dim]; bag b = ids[offsets[b]:offsets[b+1]]
    x = emb.torch_lookup(token_ids, dtype=torch.bfloat16)       # torch tensor on the device, ids from any device
    s = emb.torch_bag(token_ids, offsets, mode="sum")
    v = emb.torch_bag(token_ids, offsets, mode="mean", per_sample_weights=sif)   # weighted pooling (SIF, TF-IDF, a mask)
    logits = emb.torch_project(hidden)                          # [..., rows]: the tied output layer, from the packed rows
    scores = emb.torch_project(hidden, candidates=cand, dtype=torch.bfloat16)    # [..., m]: a candidate list only
    loss(emb.torch_project(hidden.requires_grad_())).backward() # hidden.grad comes from the packed rows too (no float table)
    mean = emb.torch_backproject(probs)                         # [..., dim]: the expected embedding probs @ E
    loss = emb.torch_xent(hidden.requires_grad_(), y, reduction="mean")   # softmax cross-entropy of the tied output layer:
    loss.backward()                                             # no [n, rows] logits, probabilities or gradient are ever held
    values, rows = emb.torch_topk(hidden, 8, log_probs=True)    # the 8 best rows per vector (beam search): no logits held either
    token = emb.torch_sample(hidden, 40, temperature=0.8)       # top-k sampling

Lookup, pooling, the projection, its back-projection, the cross-entropy and the top-k selection run on the MI355X
(w2b_kernels_embed.hip, w2b_kernels_embedproj.hip, w2b_kernels_embedback.hip, w2b_kernels_embedxent.hip,
w2b_kernels_embedtopk.hip); there is no CPU path in this module.
"""
import ctypes as C

import numpy as np

from . import _lib

DTYPES = {"float32": 0, "bfloat16": 1, "float16": 2}
MODES = {"sum": 0, "mean": 1}
MAX_BAG = 1 << 22
MAX_K = 64


def _dtype_code(dtype):
    name = str(dtype).replace("torch.", "")
    if name not in DTYPES:
        raise ValueError("dtype must be float32, bfloat16 or float16")
    return DTYPES[name]


def _mode_code(mode):
    if mode not in MODES:
        raise ValueError("mode must be 'sum' or 'mean'")
    return MODES[mode]


_PROJECT_FUNCTION = None


def _project_function():
    """The autograd hook of PackedEmbedding.torch_project, defined on first use (torch is imported lazily throughout)."""
    global _PROJECT_FUNCTION
    if _PROJECT_FUNCTION is None:
        import torch

        class PackedProject(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, emb, candidates, dtype):
                ctx.emb, ctx.candidates = emb, candidates
                ctx.x_shape, ctx.x_dtype, ctx.x_device = x.shape, x.dtype, x.device
                return emb.torch_project(x.detach(), candidates, dtype, copy=True)

            @staticmethod
            @torch.autograd.function.once_differentiable
            def backward(ctx, grad_out):
                dx = ctx.emb.torch_backproject(grad_out, ctx.candidates)
                return dx.reshape(ctx.x_shape).to(device=ctx.x_device, dtype=ctx.x_dtype), None, None, None

        _PROJECT_FUNCTION = PackedProject
    return _PROJECT_FUNCTION


_XENT_FUNCTION = None
REDUCTIONS = ("none", "mean", "sum")


def _xent_function():
    """The autograd hook of PackedEmbedding.torch_xent, defined on first use as PackedProject is."""
    global _XENT_FUNCTION
    if _XENT_FUNCTION is None:
        import torch

        class PackedXent(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, emb, target, candidates):
                loss, dx = emb._torch_xent(x.detach(), target, candidates, True)
                ctx.save_for_backward(dx)
                ctx.x_shape, ctx.x_dtype, ctx.x_device = x.shape, x.dtype, x.device
                return loss

            @staticmethod
            @torch.autograd.function.once_differentiable
            def backward(ctx, grad_out):
                dx, = ctx.saved_tensors
                g = dx * grad_out.to(device=dx.device, dtype=torch.float32).reshape(-1, 1)
                return g.reshape(ctx.x_shape).to(device=ctx.x_device, dtype=ctx.x_dtype), None, None, None

        _XENT_FUNCTION = PackedXent
    return _XENT_FUNCTION


class PackedEmbedding:
    """A read-only embedding table of a 1-bit or 2-bit model, bit-packed on the device.  Either `path` (a .w2bp file;
    `threshold` caps the rows) or `packed` (uint64 [rows, words_per_row] in the .w2bp layout, e.g. Trainer.export_packed())
    with `dim` and `bitlevel`."""

    def __init__(self, path=None, packed=None, dim=None, bitlevel=None, threshold=0, device=0):
        self._h = C.c_void_p()
        self._L = _lib.lib()
        self.device = int(device)
        if (path is None) == (packed is None):
            raise ValueError("give either path or packed")
        if path is not None:
            _lib.check(self._L.w2b_embed_load(str(path).encode(), int(threshold), self.device, C.byref(self._h)))
        else:
            if dim is None or bitlevel is None:
                raise ValueError("packed rows need dim and bitlevel")
            packed = np.ascontiguousarray(packed, np.uint64)
            wpr = int(self._L.w2b_packed_words_per_row(int(dim), int(bitlevel)))
            if wpr > 0 and (packed.ndim != 2 or packed.shape[1] != wpr):
                raise ValueError("packed must be [rows, %d] for dim %d at bitlevel %d" % (wpr, dim, bitlevel))
            _lib.check(self._L.w2b_embed_create(packed.ctypes.data_as(_lib.u64p), packed.shape[0], int(dim), int(bitlevel),
                                                self.device, C.byref(self._h)))
        self.rows = int(self._L.w2b_embed_rows(self._h))
        self.dim = int(self._L.w2b_embed_dim(self._h))
        self.bitlevel = int(self._L.w2b_embed_bitlevel(self._h))

    def close(self):
        if self._h:
            self._L.w2b_embed_free(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def word(self, row):
        """The word of `row` (bytes), None on a handle made from packed rows."""
        return self._L.w2b_embed_word(self._h, int(row))

    def search(self, word):
        """The first row whose word is exactly `word` (bytes or str), -1 if there is none."""
        return int(self._L.w2b_embed_search(self._h, word if isinstance(word, bytes) else str(word).encode()))

    # ---- host form: numpy in, numpy out
    @staticmethod
    def _out(shape, code):
        return np.empty(shape, (np.float32, np.uint16, np.float16)[code])

    def lookup(self, ids, dtype="float32"):
        """Rows of `ids` (int array, any shape; < 0 = padding): numpy ids.shape + (dim,).  float16 comes as np.float16,
        bfloat16 as np.uint16 bit patterns."""
        code = _dtype_code(dtype)
        ids = np.ascontiguousarray(ids, np.int32)
        out = self._out(ids.shape + (self.dim,), code)
        _lib.check(self._L.w2b_embed_lookup(self._h, ids.size, ids.ctypes.data_as(_lib.i32p), code,
                                            C.c_void_p(out.ctypes.data)))
        return out

    def bag(self, ids, offsets, mode="sum", dtype="float32", per_sample_weights=None):
        """Sum or mean of the rows of every bag: numpy [len(offsets) - 1, dim].  per_sample_weights (float array of ids'
        shape, cast to float32) weighs every id's row: the weighted bag of the header, whose mean still divides by the
        number of ids."""
        code, m = _dtype_code(dtype), _mode_code(mode)
        ids = np.ascontiguousarray(ids, np.int32)
        if per_sample_weights is not None and np.shape(per_sample_weights) != ids.shape:
            raise ValueError("per_sample_weights must have the shape of ids")
        ids = ids.ravel()
        offsets = np.ascontiguousarray(offsets, np.int64).ravel()
        if offsets.size < 1:
            raise ValueError("offsets has n_bags + 1 entries")
        out = self._out((offsets.size - 1, self.dim), code)
        if per_sample_weights is not None:
            w = np.ascontiguousarray(per_sample_weights, np.float32).ravel()
            _lib.check(self._L.w2b_embed_bag_weighted(self._h, ids.size, ids.ctypes.data_as(_lib.i32p),
                                                      w.ctypes.data_as(_lib.f32p), offsets.size - 1,
                                                      offsets.ctypes.data_as(_lib.i64p), m, code, C.c_void_p(out.ctypes.data)))
            return out
        _lib.check(self._L.w2b_embed_bag(self._h, ids.size, ids.ctypes.data_as(_lib.i32p), offsets.size - 1,
                                         offsets.ctypes.data_as(_lib.i64p), m, code, C.c_void_p(out.ctypes.data)))
        return out

    def project(self, x, candidates=None, dtype="float32"):
        """Logits of the vectors `x` (float array [..., dim], cast to float32) against the rows `candidates` (int array
        [m]; < 0 = padding, a column of +0.0) or against every row: numpy x.shape[:-1] + (m,).  The projection of the
        header: one float32 fmaf chain per (vector, candidate), a defined result bit for bit."""
        code = _dtype_code(dtype)
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim < 1 or x.shape[-1] != self.dim:
            raise ValueError("x must be [..., %d]" % self.dim)
        n = x.size // self.dim
        if candidates is None:
            m, cand_p = self.rows, None
        else:
            cand = np.ascontiguousarray(candidates, np.int32).ravel()
            m, cand_p = cand.size, cand.ctypes.data_as(_lib.i32p)
        out = self._out(x.shape[:-1] + (m,), code)
        _lib.check(self._L.w2b_embed_project(self._h, n, x.ctypes.data_as(_lib.f32p), m, cand_p, code,
                                             C.c_void_p(out.ctypes.data)))
        return out

    def backproject(self, g, candidates=None):
        """The back-projection of the header: dx[i] = sum over j of g[i][j] * row candidates[j] (`g` float array [..., m],
        cast to float32; candidates int array [m], < 0 = padding whose g is ignored, or every row): numpy float32
        g.shape[:-1] + (dim,).  The gradient of project() with respect to x, and the expected embedding p @ E; one defined
        result bit for bit (the weighted bag's segment rule)."""
        g = np.ascontiguousarray(g, np.float32)
        if candidates is None:
            m, cand_p = self.rows, None
        else:
            cand = np.ascontiguousarray(candidates, np.int32).ravel()
            m, cand_p = cand.size, cand.ctypes.data_as(_lib.i32p)
        if g.ndim < 1 or g.shape[-1] != m:
            raise ValueError("g must be [..., %d]" % m)
        n = int(np.prod(g.shape[:-1]))
        out = np.empty(g.shape[:-1] + (self.dim,), np.float32)
        _lib.check(self._L.w2b_embed_backproject(self._h, n, g.ctypes.data_as(_lib.f32p), m, cand_p,
                                                 out.ctypes.data_as(_lib.f32p)))
        return out

    def xent(self, x, target, candidates=None, grad=False):
        """Softmax cross-entropy of the vectors `x` (float array [..., dim], cast to float32) against the rows `candidates`
        (int array [m]; < 0 = padding) or every row: the loss as float64 x.shape[:-1], or (loss, dx) with dx float32
        x.shape when grad=True.  `target` (int array x.shape[:-1]) holds candidate POSITIONS (rows, without candidates);
        < 0 = ignored, whose loss is 0 and whose dx is +0.  The cross-entropy of the header: mx, se and tl are defined bit
        for bit, and the loss is (mx - tl) + log(se) in float64."""
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim < 1 or x.shape[-1] != self.dim:
            raise ValueError("x must be [..., %d]" % self.dim)
        target = np.ascontiguousarray(target, np.int32)
        if target.shape != x.shape[:-1]:
            raise ValueError("target must have the shape of x without its last axis")
        n = target.size
        if candidates is None:
            m, cand_p = self.rows, None
        else:
            cand = np.ascontiguousarray(candidates, np.int32).ravel()
            m, cand_p = cand.size, cand.ctypes.data_as(_lib.i32p)
        stats = np.empty((3, max(n, 1)), np.float32)
        dx = np.empty(x.shape, np.float32) if grad else None
        _lib.check(self._L.w2b_embed_xent(self._h, n, x.ctypes.data_as(_lib.f32p), m, cand_p, target.ctypes.data_as(_lib.i32p),
                                          stats[0].ctypes.data_as(_lib.f32p), stats[1].ctypes.data_as(_lib.f32p),
                                          stats[2].ctypes.data_as(_lib.f32p), None if dx is None else dx.ctypes.data_as(_lib.f32p)))
        mx, se, tl = stats[:, :n].astype(np.float64)
        live = target.ravel() >= 0
        loss = np.zeros(n, np.float64)
        loss[live] = (mx[live] - tl[live]) + np.log(se[live])
        loss = loss.reshape(target.shape)
        return (loss, dx) if grad else loss

    def topk(self, x, k, candidates=None):
        """The k largest logits of every vector of `x` (float array [..., dim], cast to float32) against the rows
        `candidates` (int array [m]; < 0 = padding, never an answer) or against every row, and where they stand: (vals
        float32, pos int32), both x.shape[:-1] + (k,), best first.  pos is a candidate POSITION (the row, without
        candidates).  The top-k of the header: logit descending, equal logits in ascending position, the values the
        projection's bit for bit; with fewer than k live positions a list ends in pos = -1, val = -inf.  1 <= k <= 64."""
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim < 1 or x.shape[-1] != self.dim:
            raise ValueError("x must be [..., %d]" % self.dim)
        n = x.size // self.dim
        if candidates is None:
            m, cand_p = self.rows, None
        else:
            cand = np.ascontiguousarray(candidates, np.int32).ravel()
            m, cand_p = cand.size, cand.ctypes.data_as(_lib.i32p)
        k = int(k)
        shape = x.shape[:-1] + (max(k, 0),)
        vals, pos = np.empty(shape, np.float32), np.empty(shape, np.int32)
        _lib.check(self._L.w2b_embed_topk(self._h, n, x.ctypes.data_as(_lib.f32p), m, cand_p, k, vals.ctypes.data_as(_lib.f32p),
                                          pos.ctypes.data_as(_lib.i32p)))
        return vals, pos

    # ---- device form: library-owned staging, viewed by torch
    def reserve(self, max_ids, max_bags=0, dtype="float32"):
        """(ids_dev, offsets_dev, out_dev) addresses of the library's staging buffers (w2b_embed_reserve)."""
        p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        _lib.check(self._L.w2b_embed_reserve(self._h, int(max_ids), int(max_bags), _dtype_code(dtype), *map(C.byref, p)))
        return tuple(x.value for x in p)

    def lookup_device(self, n, dtype="float32"):
        _lib.check(self._L.w2b_embed_lookup_device(self._h, int(n), _dtype_code(dtype)))

    def bag_device(self, n_ids, n_bags, mode="sum", dtype="float32"):
        _lib.check(self._L.w2b_embed_bag_device(self._h, int(n_ids), int(n_bags), _mode_code(mode), _dtype_code(dtype)))

    def reserve_weights(self, max_ids):
        """Address of the library's float32 [max_ids] weights buffer (w2b_embed_reserve_weights); it moves only when it
        grows itself."""
        p = C.c_void_p()
        _lib.check(self._L.w2b_embed_reserve_weights(self._h, int(max_ids), C.byref(p)))
        return p.value

    def bag_weighted_device(self, n_ids, n_bags, mode="sum", dtype="float32"):
        _lib.check(self._L.w2b_embed_bag_weighted_device(self._h, int(n_ids), int(n_bags), _mode_code(mode),
                                                         _dtype_code(dtype)))

    def reserve_project(self, max_n, max_m, dtype="float32"):
        """(x_dev, cand_dev, out_dev) addresses of the projection's staging buffers (w2b_embed_reserve_project): buffers of
        their own, each of which moves only when it grows itself."""
        p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        _lib.check(self._L.w2b_embed_reserve_project(self._h, int(max_n), int(max_m), _dtype_code(dtype), *map(C.byref, p)))
        return tuple(x.value for x in p)

    def project_device(self, n, m, use_candidates=True, dtype="float32"):
        _lib.check(self._L.w2b_embed_project_device(self._h, int(n), int(m), 1 if use_candidates else 0, _dtype_code(dtype)))

    def reserve_backproject(self, max_n, max_m):
        """(g_dev, cand_dev, dx_dev) addresses of the back-projection's staging buffers (w2b_embed_reserve_backproject):
        buffers of their own, each of which moves only when it grows itself."""
        p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        _lib.check(self._L.w2b_embed_reserve_backproject(self._h, int(max_n), int(max_m), *map(C.byref, p)))
        return tuple(x.value for x in p)

    def backproject_device(self, n, m, use_candidates=True):
        _lib.check(self._L.w2b_embed_backproject_device(self._h, int(n), int(m), 1 if use_candidates else 0))

    def reserve_xent(self, max_n, max_m):
        """(x_dev, cand_dev, target_dev, stats_dev, dx_dev) addresses of the cross-entropy's staging buffers
        (w2b_embed_reserve_xent): buffers of their own, each of which moves only when it grows itself."""
        p = [C.c_void_p() for _ in range(5)]
        _lib.check(self._L.w2b_embed_reserve_xent(self._h, int(max_n), int(max_m), *map(C.byref, p)))
        return tuple(x.value for x in p)

    def xent_device(self, n, m, use_candidates=True, want_dx=False):
        _lib.check(self._L.w2b_embed_xent_device(self._h, int(n), int(m), 1 if use_candidates else 0, 1 if want_dx else 0))

    def reserve_topk(self, max_n, max_m, max_k):
        """(x_dev, cand_dev, vals_dev, pos_dev) addresses of the top-k selection's staging buffers (w2b_embed_reserve_topk):
        buffers of their own, each of which moves only when it grows itself."""
        p = [C.c_void_p() for _ in range(4)]
        _lib.check(self._L.w2b_embed_reserve_topk(self._h, int(max_n), int(max_m), int(max_k), *map(C.byref, p)))
        return tuple(x.value for x in p)

    def topk_device(self, n, m, k, use_candidates=True):
        _lib.check(self._L.w2b_embed_topk_device(self._h, int(n), int(m), 1 if use_candidates else 0, int(k)))

    def synchronize(self):
        _lib.check(self._L.w2b_embed_synchronize(self._h))

    def bad_ids(self):
        """Ids >= rows, clamped bags and refused weights that the device form has ignored since the last call
        (synchronises, resets)."""
        n = C.c_int64()
        _lib.check(self._L.w2b_embed_bad_ids(self._h, C.byref(n)))
        return n.value

    def _view(self, ptr, count, typestr):
        """torch view (no copy) of `count` elements of a library-owned device buffer (as Trainer.model_tensor)"""
        import torch

        class _View:
            __cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False), "version": 2}
        return torch.as_tensor(_View(), device=torch.device("cuda", self.device))

    def staging(self, max_ids, max_bags=0, dtype="float32"):
        """torch views of the staging buffers: ids int64 [max_ids], offsets int64 [max_bags + 1], out [max(max_ids,
        max_bags), dim] of `dtype`; valid until a later call reserves more."""
        import torch
        code = _dtype_code(dtype)
        ids_p, off_p, out_p = self.reserve(max_ids, max_bags, dtype)
        nout = max(int(max_ids), int(max_bags))
        out = self._view(out_p, max(nout * self.dim, 1), ("<f4", "<i2", "<f2")[code])
        if code == 1:
            out = out.view(torch.bfloat16)
        return (self._view(ids_p, max(int(max_ids), 1), "<i8")[:int(max_ids)],
                self._view(off_p, int(max_bags) + 1, "<i8"), out[:nout * self.dim].view(nout, self.dim))

    def staging_weights(self, max_ids):
        """torch view of the weights buffer: float32 [max_ids]; valid until a later call reserves more weights."""
        return self._view(self.reserve_weights(max_ids), max(int(max_ids), 1), "<f4")[:int(max_ids)]

    def staging_project(self, max_n, max_m, dtype="float32"):
        """torch views of the projection's staging buffers: x float32 [max_n, dim], candidates int64 [max_m], out flat
        [max_n * max_m] of `dtype` (a call of n vectors and m candidates leaves out[:n * m].view(n, m)); each valid until
        a later call makes that buffer grow."""
        import torch
        code = _dtype_code(dtype)
        max_n, max_m = int(max_n), int(max_m)
        x_p, cand_p, out_p = self.reserve_project(max_n, max_m, dtype)
        out = self._view(out_p, max(max_n * max_m, 1), ("<f4", "<i2", "<f2")[code])
        if code == 1:
            out = out.view(torch.bfloat16)
        return (self._view(x_p, max(max_n * self.dim, 1), "<f4")[:max_n * self.dim].view(max_n, self.dim),
                self._view(cand_p, max(max_m, 1), "<i8")[:max_m], out[:max_n * max_m])

    def staging_backproject(self, max_n, max_m):
        """torch views of the back-projection's staging buffers: g float32 flat [max_n * max_m] (a call of n vectors and m
        candidates reads g[:n * m].view(n, m)), candidates int64 [max_m], dx float32 [max_n, dim]; each valid until a later
        call makes that buffer grow."""
        max_n, max_m = int(max_n), int(max_m)
        g_p, cand_p, dx_p = self.reserve_backproject(max_n, max_m)
        return (self._view(g_p, max(max_n * max_m, 1), "<f4")[:max_n * max_m],
                self._view(cand_p, max(max_m, 1), "<i8")[:max_m],
                self._view(dx_p, max(max_n * self.dim, 1), "<f4")[:max_n * self.dim].view(max_n, self.dim))

    def staging_xent(self, max_n, max_m):
        """torch views of the cross-entropy's staging buffers: x float32 [max_n, dim], candidates int64 [max_m], target
        int64 [max_n], stats float32 flat [3 * max_n] (a call of n vectors leaves stats[:3 * n].view(3, n): mx, se, tl), dx
        float32 [max_n, dim]; each valid until a later call makes that buffer grow."""
        max_n, max_m = int(max_n), int(max_m)
        x_p, cand_p, tgt_p, stats_p, dx_p = self.reserve_xent(max_n, max_m)
        rows = lambda p: self._view(p, max(max_n * self.dim, 1), "<f4")[:max_n * self.dim].view(max_n, self.dim)
        return (rows(x_p), self._view(cand_p, max(max_m, 1), "<i8")[:max_m], self._view(tgt_p, max(max_n, 1), "<i8")[:max_n],
                self._view(stats_p, max(3 * max_n, 1), "<f4")[:3 * max_n], rows(dx_p))

    def staging_topk(self, max_n, max_m, max_k):
        """torch views of the top-k selection's staging buffers: x float32 [max_n, dim], candidates int64 [max_m], vals
        float32 and pos int64, both flat [max_n * max_k] (a call of n vectors and k answers leaves vals[:n * k].view(n, k)
        and pos[:n * k].view(n, k)); each valid until a later call makes that buffer grow."""
        max_n, max_m, max_k = int(max_n), int(max_m), int(max_k)
        x_p, cand_p, vals_p, pos_p = self.reserve_topk(max_n, max_m, max_k)
        return (self._view(x_p, max(max_n * self.dim, 1), "<f4")[:max_n * self.dim].view(max_n, self.dim),
                self._view(cand_p, max(max_m, 1), "<i8")[:max_m],
                self._view(vals_p, max(max_n * max_k, 1), "<f4")[:max_n * max_k],
                self._view(pos_p, max(max_n * max_k, 1), "<i8")[:max_n * max_k])

    def _finish(self, out, copy, what):
        self.synchronize()
        bad = self.bad_ids()
        if bad:
            raise _lib.W2bError(_lib.W2B_EINVAL, "%s: %d ids >= rows, bag bounds outside the ids or weights out of range" % (what, bad))
        return out.clone() if copy else out

    def torch_lookup(self, ids, dtype=None, copy=True):
        """Rows of `ids` (torch integer tensor on any device): tensor ids.shape + (dim,) on this handle's device.
        copy=False returns the view of the library's buffer, valid until the next call on this handle."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        n = ids.numel()
        ids_t, _, out = self.staging(n, 0, dtype)
        if n:
            ids_t.copy_(ids.reshape(-1))
            torch.cuda.synchronize()                  # the library's stream does not wait for torch's
            self.lookup_device(n, dtype)
        return self._finish(out[:n].view(tuple(ids.shape) + (self.dim,)), copy, "torch_lookup")

    def torch_bag(self, ids, offsets, mode="sum", dtype=None, copy=True, per_sample_weights=None):
        """Sum or mean per bag (torch integer tensors on any device; offsets has n_bags + 1 entries): [n_bags, dim].
        per_sample_weights (float tensor of ids' shape on any device, cast to float32) as in PackedEmbedding.bag."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        n, nb = ids.numel(), offsets.numel() - 1
        if nb < 0:
            raise ValueError("offsets has n_bags + 1 entries")
        if per_sample_weights is not None and tuple(per_sample_weights.shape) != tuple(ids.shape):
            raise ValueError("per_sample_weights must have the shape of ids")
        ids_t, off_t, out = self.staging(n, nb, dtype)
        w_t = self.staging_weights(n) if per_sample_weights is not None else None
        if nb:
            if n:
                ids_t.copy_(ids.reshape(-1))
                if w_t is not None:
                    w_t.copy_(per_sample_weights.reshape(-1))             # copy_ casts to float32
            off_t.copy_(offsets.reshape(-1))
            torch.cuda.synchronize()
            if w_t is not None:
                self.bag_weighted_device(n, nb, mode, dtype)
            else:
                self.bag_device(n, nb, mode, dtype)
        return self._finish(out[:nb], copy, "torch_bag")

    def torch_project(self, x, candidates=None, dtype=None, copy=True):
        """Logits of `x` (torch tensor [..., dim] on any device, cast to float32) against `candidates` (integer tensor [m]
        on any device, cast to int64) or every row: tensor x.shape[:-1] + (m,) on this handle's device.  A candidate >=
        rows raises; copy=False returns the view of the library's buffer, valid until the next call on this handle.
        Differentiable with respect to x, once: when x requires a gradient (and grad mode is on) the result is a copy that
        carries a grad_fn, whose backward is torch_backproject of the incoming gradient (cast to float32), returned with
        x's shape, dtype and device.  The table gets no gradient."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if x.dim() < 1 or x.shape[-1] != self.dim:
            raise ValueError("x must be [..., %d]" % self.dim)
        if x.requires_grad and torch.is_grad_enabled():
            return _project_function().apply(x, self, candidates, dtype)
        n = x.numel() // self.dim
        m = self.rows if candidates is None else candidates.numel()
        x_t, cand_t, out = self.staging_project(n, m, dtype)
        if n and m:
            x_t.copy_(x.reshape(n, self.dim))                 # copy_ casts to float32
            if candidates is not None:
                cand_t.copy_(candidates.reshape(-1))
            torch.cuda.synchronize()                          # the library's stream does not wait for torch's
            self.project_device(n, m, candidates is not None, dtype)
        return self._finish(out[:n * m].view(tuple(x.shape[:-1]) + (m,)), copy, "torch_project")

    def torch_backproject(self, g, candidates=None, copy=True):
        """The back-projection of `g` (torch tensor [..., m] on any device, cast to float32) through `candidates` (integer
        tensor [m] on any device, cast to int64; < 0 = padding whose g is ignored) or every row: float32 tensor
        g.shape[:-1] + (dim,) on this handle's device.  A candidate >= rows raises; copy=False returns the view of the
        library's buffer, valid until the next call on this handle."""
        import torch
        m = self.rows if candidates is None else candidates.numel()
        if g.dim() < 1 or g.shape[-1] != m:
            raise ValueError("g must be [..., %d]" % m)
        n = g.numel() // m if m else int(np.prod(tuple(g.shape[:-1])))
        g_t, cand_t, dx = self.staging_backproject(n, m)
        if n:
            if m:
                g_t[:n * m].view(n, m).copy_(g.reshape(n, m))     # copy_ casts to float32
                if candidates is not None:
                    cand_t.copy_(candidates.reshape(-1))
            torch.cuda.synchronize()                              # the library's stream does not wait for torch's
            self.backproject_device(n, m, candidates is not None or m == 0)
        return self._finish(dx[:n].view(tuple(g.shape[:-1]) + (self.dim,)), copy, "torch_backproject")

    def _torch_xent(self, x, target, candidates, want_dx):
        """(loss float32 [n] = (mx - tl) + log(se), 0 for an ignored vector; dx float32 [n, dim] or None), copies"""
        import torch
        n = x.numel() // self.dim
        m = self.rows if candidates is None else candidates.numel()
        x_t, cand_t, tgt_t, stats, dx = self.staging_xent(n, m)
        if n:
            x_t.copy_(x.reshape(n, self.dim))                     # copy_ casts to float32
            tgt_t.copy_(target.reshape(-1))
            if candidates is not None and m:
                cand_t.copy_(candidates.reshape(-1))
            torch.cuda.synchronize()                              # the library's stream does not wait for torch's
            self.xent_device(n, m, candidates is not None or m == 0, want_dx)
        mx, se, tl = self._finish(stats[:3 * n].view(3, n), True, "torch_xent")
        live = tgt_t >= 0
        loss = torch.where(live, (mx - tl) + torch.log(torch.where(live, se, torch.ones_like(se))), torch.zeros_like(se))
        return loss, (dx[:n].clone() if want_dx else None)

    def torch_xent(self, x, target, candidates=None, reduction="none"):
        """Softmax cross-entropy of `x` (torch tensor [..., dim] on any device, cast to float32) against `candidates`
        (integer tensor [m] on any device; < 0 = padding) or every row, with `target` (integer tensor x.shape[:-1]) the
        candidate POSITION of every vector (the row, without candidates; < 0 = ignored): float32 on this handle's device,
        x.shape[:-1] for reduction "none", a scalar for "sum" and for "mean", which divides by the number of vectors that
        are not ignored, as torch does.  A candidate >= rows, a target >= m or one on a padding position raises.
        Differentiable with respect to x, once: when x requires a gradient (and grad mode is on) the call also computes dx
        on the device -- without a [n, m] array -- and backward returns dx times the incoming gradient, with x's shape,
        dtype and device.  The table gets no gradient."""
        import torch
        if reduction not in REDUCTIONS:
            raise ValueError("reduction must be 'none', 'mean' or 'sum'")
        if x.dim() < 1 or x.shape[-1] != self.dim:
            raise ValueError("x must be [..., %d]" % self.dim)
        if tuple(target.shape) != tuple(x.shape[:-1]):
            raise ValueError("target must have the shape of x without its last axis")
        if x.requires_grad and torch.is_grad_enabled():
            loss = _xent_function().apply(x, self, target, candidates)
        else:
            loss = self._torch_xent(x, target, candidates, False)[0]
        if reduction == "none":
            return loss.reshape(tuple(target.shape))
        if reduction == "sum":
            return loss.sum()
        count = (target >= 0).sum().to(device=loss.device, dtype=torch.float32)
        return loss.sum() / count

    def torch_topk(self, x, k, candidates=None, log_probs=False, copy=True):
        """(values float32, indices int64), both x.shape[:-1] + (k,) on this handle's device, in the shape of torch.topk:
        the k largest logits of `x` (torch tensor [..., dim] on any device, cast to float32) against `candidates` (integer
        tensor [m] on any device; < 0 = padding, never an answer) or every row, best first, and the candidate POSITIONS
        they stand at (the rows, without candidates).  The top-k of the header: no [n, m] logits are held, the values are
        torch_project's bit for bit, equal logits come in ascending position, and with fewer than k live positions a
        list ends in index -1, value -inf.  NOT differentiable: the result carries no grad_fn, whatever x requires.
        log_probs=True turns the values into log-probabilities normalised over ALL live candidates, l - mx - log(se) in
        float32 with torch.log, mx and se from one statistics call of the cross-entropy over the same operands with every
        target ignored (one more pass over the table; the logarithm is outside the bit-for-bit contract, as in
        torch_xent); entries with index -1 stay -inf.  A candidate >= rows raises; copy=False returns views of the library's buffers, valid until the next
        call on this handle (with log_probs the values are always a new tensor)."""
        import torch
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("k must be within 1 .. %d" % MAX_K)
        if x.dim() < 1 or x.shape[-1] != self.dim:
            raise ValueError("x must be [..., %d]" % self.dim)
        x = x.detach()
        n = x.numel() // self.dim
        m = self.rows if candidates is None else candidates.numel()
        x_t, cand_t, vals, pos = self.staging_topk(n, m, k)
        if n:
            x_t.copy_(x.reshape(n, self.dim))                     # copy_ casts to float32
            if candidates is not None and m:
                cand_t.copy_(candidates.reshape(-1))
            torch.cuda.synchronize()                              # the library's stream does not wait for torch's
            self.topk_device(n, m, k, candidates is not None or m == 0)
        shape = tuple(x.shape[:-1]) + (k,)
        values = self._finish(vals[:n * k].view(shape), copy, "torch_topk")
        indices = pos[:n * k].view(shape)
        indices = indices.clone() if copy else indices
        if log_probs and n:
            # mx and se of every vector: the statistics of the cross-entropy with every target ignored
            xs, cs, tgt, stats, _ = self.staging_xent(n, m)
            xs.copy_(x_t[:n])
            tgt.fill_(-1)
            if candidates is not None and m:
                cs.copy_(cand_t[:m])
            torch.cuda.synchronize()
            self.xent_device(n, m, candidates is not None or m == 0, False)
            mx, se, _ = self._finish(stats[:3 * n].view(3, n), True, "torch_topk")
            one = shape[:-1] + (1,)                               # (se is 0 only where nothing is live: all indices -1)
            log_se = torch.log(torch.where(se > 0, se, torch.ones_like(se)))
            values = torch.where(indices >= 0, (values - mx.reshape(one)) - log_se.reshape(one),
                                 torch.full_like(values, float("-inf")))
        return values, indices

    def torch_sample(self, x, k, temperature=1.0, generator=None):
        """Top-k sampling over every row: per vector of `x` one row, drawn from the softmax of the k largest logits divided
        by `temperature`: int64 x.shape[:-1] on this handle's device.  Plain torch on top of torch_topk: softmax over the k values, then torch.multinomial with
        `generator`.  k = 1 is greedy decoding.  A vector with no live candidate returns -1."""
        import torch
        if not temperature > 0:
            raise ValueError("temperature must be positive")
        values, indices = self.torch_topk(x, k)
        shape = indices.shape[:-1]
        values, indices = values.reshape(-1, indices.shape[-1]), indices.reshape(-1, indices.shape[-1])
        if values.shape[0] == 0:
            return indices[:, 0].reshape(shape)
        dead = indices[:, 0] < 0
        safe = torch.where(dead[:, None], torch.zeros_like(values), values)     # a row of -inf has no softmax
        probs = torch.softmax(safe / float(temperature), dim=1)
        pick = torch.multinomial(probs, 1, generator=generator)
        out = torch.gather(indices, 1, pick)[:, 0]
        return torch.where(dead, torch.full_like(out, -1), out).reshape(shape)

    def timing(self):
        """(kernel ms, launches, bytes moved: packed words (and weights) read + output written) since the last call."""
        ms, n, b = C.c_double(), C.c_int64(), C.c_double()
        _lib.check(self._L.w2b_embed_timing_read(self._h, C.byref(ms), C.byref(n), C.byref(b)))
        return ms.value, n.value, b.value
