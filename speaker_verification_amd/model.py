"""C3D2 speaker-embedding network (`/root/reference/model.py:104-191`): the PyTorch module -- what checkpoints load
into and what training differentiates -- and `FusedEmbedder`, its inference form: seven hand-written MFMA entry points of
libsvk (`svk_c3d2_stage1`, `svk_c3d2_stage2`, `svk_c3d2_conv31`, `svk_c3d2_conv32t`, `svk_c3d2_conv41`: csrc/c3d2.hip, two-piece
f16 products; `svk_c3d2_conv42`, `svk_c3d2_fc5`: csrc/c3d2_tail.hip, f32).

Same constructor arguments, same sub-module names (a reference-format checkpoint's `state_dict` loads unchanged), same
`forward(x, development=True)`, `load_checkpoint(d)` and `create_Speaker_Model(u)` as the reference.  Input convention
`(batch, 1, 20, 80, 40)` (`/root/reference/utils.py:368-379`), or `(batch, 3, 20, 80, 40)` for `C3D2(n, 3)` (static, delta and
delta-delta features: `utils.FeatureCube3C`, `/root/reference/utils.py:325-348`).

Which code runs a forward:
  * eval mode, input on the GPU, one-channel 20 x 80 x 40 cubes, no gradient asked of the input -- what
    `evaluation.py:67-84,113-121` and `model.py:188-191,374-388` do -- : the libsvk kernels.  A cube IS a feature
    matrix of 1 600 rows with crop starts 0, 80, 160 ...: `svk_c3d2_stage1` reads it as such, nothing is copied;
  * the same for three-channel cubes of a `C3D2(n, 3)` when `model.three_channel_kernels = True` (on the instance or the
    class): `svk_c3d2_stage1_c3` reads the cube as three planes of 1 600 rows.  Off by default, so that forward's routing
    stays what it was; `FusedEmbedder(model)` and `evaluation.dataset_embeddings` take the kernels for three channels as
    they do for one;
  * training mode, gradients, other channel counts, tensors on the host: the torch layers
    (autograd needs them; the north-star leaves the training forward on PyTorch-ROCm).
`model.inference_kernels = False` keeps an instance on the torch layers (A/B comparisons in tools).

The classification head of `forward(x, development=True)` (PReLU5 -> FC6 -> softmax, model.py:170-174) runs on torch operators
unless `model.head_kernels = True`, which sends it to `svk_c3d2_head` (csrc/head.hip) whenever the network itself runs on the
kernels; `identify` (top-k labels, the accuracy pass of train.py:104-119) uses that kernel wherever the kernels apply.
"""
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

# name suffix, in_ch (None = num_channels), out_ch, kernel, stride, maxpool after
_LAYERS = (
    ("1_1", None, 16, (3, 1, 5), (1, 1, 1), False),
    ("1_2", 16, 16, (3, 9, 1), (1, 2, 1), True),
    ("2_1", 16, 32, (3, 1, 4), (1, 1, 1), False),
    ("2_2", 32, 32, (3, 8, 1), (1, 2, 1), True),
    ("3_1", 32, 64, (3, 1, 3), (1, 1, 1), False),
    ("3_2", 64, 64, (3, 7, 1), (1, 1, 1), False),
    ("4_1", 64, 128, (3, 1, 3), (1, 1, 1), False),
    ("4_2", 128, 128, (3, 7, 1), (1, 1, 1), False),
)
EMBED_DIM = 128
_FLAT = 4 * 3 * 3 * 128
CUBE_SHAPE = (1, 20, 80, 40)          # channel, crops, frames, coefficients (utils.py:20-21, 368-379)
_EMBEDDERS = weakref.WeakKeyDictionary()   # model -> (state key, FusedEmbedder): kept off the module (deepcopy / pickling stay plain)
_HEADS = weakref.WeakKeyDictionary()       # model -> (head key, FusedHead), the same way


class C3D2(nn.Module):
    inference_kernels = True          # False on an instance: forward stays on the torch layers whatever the mode
    three_channel_kernels = False     # True on an instance (or the class): forward runs three-channel cubes on the kernels too
    head_kernels = False              # True: forward(x, development=True) takes its softmax from svk_c3d2_head when x runs on the kernels

    def __init__(self, n_labels, num_channels):
        super().__init__()
        self.n_labels, self.num_channels = n_labels, num_channels
        # creation order = the reference's, so that the same torch seed draws
        # the same initial weights (model.py:110-139)
        for tag, cin, cout, kernel, stride, pool in _LAYERS:
            cin = num_channels if cin is None else cin
            setattr(self, "conv" + tag, nn.Conv3d(cin, cout, kernel_size=kernel, stride=stride))
            setattr(self, "batch_norm" + tag, nn.BatchNorm3d(num_features=cout))
            setattr(self, "PReLu" + tag, nn.PReLU())
            if pool:
                setattr(self, "pool" + tag[0], nn.MaxPool3d(kernel_size=(1, 1, 2), stride=(1, 1, 2)))
        self.FC5 = nn.Linear(_FLAT, EMBED_DIM)
        self.PReLu5 = nn.PReLU()
        self.FC6 = nn.Linear(EMBED_DIM, n_labels)

    def torch_layers(self, x):
        """conv -> BatchNorm -> PReLU (-> pool) x 8 -> FC5 on torch operators (model.py:141-169): training, autograd,
        host tensors, three-channel cubes unless `three_channel_kernels`."""
        for tag, _, _, _, _, pool in _LAYERS:
            x = getattr(self, "conv" + tag)(x)
            x = getattr(self, "batch_norm" + tag)(x)
            x = getattr(self, "PReLu" + tag)(x)
            if pool:
                x = getattr(self, "pool" + tag[0])(x)
        return self.FC5(x.view(-1, _FLAT))

    def runs_on_kernels(self, x):
        """True when forward(x) is an inference call the libsvk network covers (see the module docstring)."""
        return bool(self.inference_kernels and not self.training and isinstance(x, torch.Tensor) and x.is_cuda
                    and x.dim() == 5 and (self.num_channels == 1 or (self.num_channels == 3 and self.three_channel_kernels))
                    and tuple(x.shape[1:]) == (self.num_channels,) + CUBE_SHAPE[1:] and x.dtype == torch.float32
                    and not (torch.is_grad_enabled() and x.requires_grad))

    def forward(self, x, development=True):
        if self.runs_on_kernels(x):
            x = self.fused_inference()(x)
            if development and self.head_kernels:
                return self.fused_head()(x, probs=True, k=None)[0]
        else:
            x = self.torch_layers(x)
        if development:
            x = F.softmax(self.FC6(self.PReLu5(x)), dim=1)
        return x

    def _embeddings_on_kernels(self, emb):
        """True when `identify` may hand the embeddings [n, 128] to svk_c3d2_head: forward's routing rules for a tensor that
        is already FC5's output."""
        return bool(self.inference_kernels and not self.training and isinstance(emb, torch.Tensor) and emb.is_cuda
                    and emb.dim() == 2 and emb.shape[1] == EMBED_DIM and emb.dtype == torch.float32
                    and not (torch.is_grad_enabled() and emb.requires_grad))

    def identify(self, x, k=1, true_idx=None):
        """The top-k speakers of each input, most probable first: cubes as forward takes them, or embeddings [n, 128].
        Returns (top-k int32 [n, k], hits): hits[r] = inputs whose true_idx ([n], -1 = unknown) is among their first r + 1
        labels, None without true_idx.  On svk_c3d2_head (no probability matrix is written) where the kernels apply; elsewhere
        torch's softmax and a stable sort, ties to the lower label as the kernel breaks them."""
        with torch.no_grad():
            if x.dim() == 2:
                emb, on_kernels = x, self._embeddings_on_kernels(x)
            elif self.runs_on_kernels(x):
                emb, on_kernels = self.fused_inference()(x), True
            else:
                emb, on_kernels = self.torch_layers(x), False
            if on_kernels:
                _, top, hits = self.fused_head()(emb, probs=False, k=k, true_idx=true_idx)
                return top, hits
            p = F.softmax(self.FC6(self.PReLu5(emb)), dim=1)
            top = torch.sort(p, dim=1, descending=True, stable=True)[1][:, :k].to(torch.int32)
            if true_idx is None:
                return top, None
            t = torch.as_tensor(true_idx, device=top.device).reshape(-1, 1).long()
            first = (top.long() == t).long().cumsum(1).clamp(max=1)       # 1 from the true label's rank on
            return top, [int(v) for v in first.sum(0)]

    def load_checkpoint(self, checkpoint_dict):
        """New model with `checkpoint_dict["state_dict"]` loaded; `module.`
        prefixes left by DataParallel are stripped (model.py:177-186)."""
        model = C3D2(n_labels=self.n_labels, num_channels=self.num_channels)
        if torch.cuda.is_available():
            model.cuda()
        wanted = model.state_dict()
        loaded = {}
        for key, value in checkpoint_dict["state_dict"].items():
            key = key.replace("module.", "")
            if key in wanted:
                loaded[key] = value
        model.load_state_dict(loaded)
        return model

    def create_Speaker_Model(self, utterance):
        self.eval()
        return self.forward(utterance, development=False)

    # ---- MI355X inference path -------------------------------------------
    def _state_key(self):
        """Identity and version of every tensor the embedding depends on: in-place updates (an optimiser step,
        load_state_dict) bump `_version`, `.to(device)` changes the storage."""
        return tuple((k, v.data_ptr(), v._version) for k, v in self.state_dict(keep_vars=True).items()
                     if not k.startswith(("FC6", "PReLu5")))

    def fused_inference(self):
        """The embedding-only inference form of the CURRENT weights (eval-mode BatchNorm folded into the convolutions,
        operands in the kernels' lane order): same maths as forward(development=False).  Cached until a weight changes."""
        key = self._state_key()
        hit = _EMBEDDERS.get(self)
        if hit is None or hit[0] != key:
            hit = _EMBEDDERS[self] = (key, FusedEmbedder(self))
        return hit[1]

    def _head_key(self):
        """Identity and version of the head's tensors (FC6.*, PReLu5.*), which `_state_key` leaves out."""
        return tuple((k, v.data_ptr(), v._version) for k, v in self.state_dict(keep_vars=True).items()
                     if k.startswith(("FC6", "PReLu5")))

    def fused_head(self):
        """The classification head of the CURRENT weights for svk_c3d2_head: FC6's weight and bias as f32 tables, PReLu5's
        slope.  Cached under its own key: a change to FC6 or PReLu5 rebuilds it, a change elsewhere does not."""
        key = self._head_key()
        hit = _HEADS.get(self)
        if hit is None or hit[0] != key:
            hit = _HEADS[self] = (key, FusedHead(self))
        return hit[1]


class FusedHead:
    """model.py:170-174's PReLU5 -> FC6 -> softmax as svk_c3d2_head; a snapshot of the weights at build time."""

    def __init__(self, model):
        if model.PReLu5.weight.numel() != 1 or tuple(model.FC6.weight.shape[1:]) != (EMBED_DIM,):
            raise ValueError("svk_c3d2_head takes FC6 (128 -> n_labels) behind a one-slope PReLU5 (model.py:138-139)")
        with torch.no_grad():
            self.w6 = model.FC6.weight.detach().to(torch.float32).contiguous().clone()
            self.b6 = model.FC6.bias.detach().to(torch.float32).contiguous().clone()
            self.slope = float(model.PReLu5.weight.detach().reshape(()))
        self.n_labels = int(self.w6.shape[0])
        self.device = self.w6.device

    def tables(self):
        return self.w6, self.b6, self.slope

    @torch.no_grad()
    def __call__(self, emb, probs=True, k=1, true_idx=None):
        """embeddings [n, 128] on the device -> (probs [n, n_labels] | None, top-k int32 [n, k] | None, hits | None)."""
        if self.device.type != "cuda":
            raise RuntimeError("svk_c3d2_head runs on the GPU; move the model to the device -- there is no CPU fallback")
        from .engine import get_engine
        return get_engine(self.device.index).c3d2_head(emb, self.tables(), probs=probs, k=k, true_idx=true_idx)


class FusedEmbedder:
    """C3D2's forward(development=False) as seven libsvk kernels; the weights are a snapshot of the model at build time.
    Built for C3D2's layer shapes on one- or three-channel cubes only: anything else raises (no framework fallback here -- the
    torch module itself is the path for other shapes)."""

    def __init__(self, model):
        self.device = model.conv1_1.weight.device       # tables are built where the weights live; kernels need the GPU
        self.num_channels = int(model.conv1_1.weight.shape[1])
        if self.num_channels not in (1, 3) or tuple(model.FC5.weight.shape) != (EMBED_DIM, _FLAT) or any(
                tuple(getattr(model, "conv" + tag).weight.shape) != (cout, self.num_channels if cin is None else cin) + kernel
                or tuple(getattr(model, "conv" + tag).stride) != stride for tag, cin, cout, kernel, stride, _ in _LAYERS):
            raise ValueError("libsvk's network kernels are built for C3D2's layers on one- or three-channel 20 x 80 x 40 cubes "
                             "(model.py:110-139); this model's layers differ")
        self._eng = None
        self.stages = []
        self.act_scale = []     # per layer: the power of two per channel its output is carried in (all ones for an ordinary checkpoint)
        with torch.no_grad():
            s_in = None
            for tag, _, _, _, stride, pool in _LAYERS:
                conv = getattr(model, "conv" + tag)
                bn = getattr(model, "batch_norm" + tag)
                act = getattr(model, "PReLu" + tag)
                scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
                w = conv.weight * scale.view(-1, 1, 1, 1, 1)
                b = (conv.bias - bn.running_mean) * scale + bn.bias
                # Activations travel as half pairs (include/svk.h): 22 bits while a value's pieces are normal halves, an absolute
                # floor of 2^-25 below 2^-3 and nothing above 65 504.  A network is the same function when channel c of a layer is
                # scaled by a > 0 (its BatchNorm's gamma and beta times a -- PReLU and the pools are positively homogeneous) and
                # the next layer's weights on that channel by 1 / a; the pieces are not.  So the channel's scale is FIXED here: its
                # activations are carried times 2^k with k = -round(log2(|gamma| + |beta|)) (the channel's spread and offset
                # behind BatchNorm), the next layer takes 2^-k into its weights -- exact in f32, k = 0 for every channel of a
                # checkpoint trained from PyTorch's initialisation, and FC5 takes the last layer's.
                # (round(log2 m) from m's own exponent and mantissa: the same k shift for m and 2^j m, whatever log2 rounds to)
                mant, expo = torch.frexp((bn.weight.abs() + bn.bias.abs()).float().clamp(min=2.0 ** -40, max=2.0 ** 40))
                k = -(expo - (mant < 0.5 ** 0.5).to(expo.dtype))
                s_out = torch.exp2(k.to(torch.float32))
                w = w * s_out.view(-1, 1, 1, 1, 1)
                b = b * s_out
                if s_in is not None:
                    w = w / s_in.view(1, -1, 1, 1, 1)
                self.stages.append((w.contiguous(), b.contiguous(), act.weight.detach().clone(), tuple(conv.stride), pool))
                self.act_scale.append(s_out)
                s_in = s_out
            # model.py:168 flattens NCDHW: column = channel * positions + position
            fc_w = model.FC5.weight.detach()
            self.fc_w = (fc_w.view(EMBED_DIM, s_in.numel(), -1) / s_in.view(1, -1, 1)).reshape(fc_w.shape).contiguous()
            self.fc_b = model.FC5.bias.detach().clone()
            for w, b, *_ in self.stages:
                if not (bool(torch.isfinite(w).all()) and bool(torch.isfinite(b).all()) and float(w.abs().max()) < 65504.0):
                    raise ValueError("a BatchNorm-folded weight of this checkpoint is not finite or exceeds 65 504: outside what "
                                     "libsvk's half-pair operands represent")
            st = self.stages
            self._tables = {"stage1": _stage1_tables(st[0], st[1]), "stage2": _stage2_tables(st[2], st[3]),
                            "conv31": _conv31_tables(st[4]), "conv32t": _conv32t_tables(st[5]), "conv41": _conv41_tables(st[6]),
                            "conv42": _conv42_tables(st[7]), "fc5": _fc5_tables(self.fc_w, self.fc_b)}
        self._starts = {}

    @property
    def eng(self):
        if self._eng is None:
            if self.device.type != "cuda":
                raise RuntimeError("FusedEmbedder runs on the GPU (libsvk); move the model to the device -- there is no CPU fallback")
            from .engine import get_engine
            self._eng = get_engine(self.device.index)
        return self._eng

    def crop_starts(self, n, device):
        """[n, 20] int32: 0, 80, 160 ... -- a cube read as 1 600 feature rows."""
        hit = self._starts.get(n)
        if hit is None:
            from . import constants as c
            row = torch.arange(c.CUBE_CROPS, dtype=torch.int32, device=device) * c.CUBE_FRAMES
            hit = self._starts[n] = row[None, :].expand(n, -1).contiguous()
            if len(self._starts) > 8:
                self._starts.pop(next(iter(self._starts)))
        return hit

    @torch.no_grad()
    def embed_features(self, feat, crop_idx, timed=None, pool=None):
        """feature rows [n, T, 40] (one-channel model) or [n, 3, T, 40] (three-channel: static, delta, delta-delta) + crop
        starts [n, 20] -> embeddings [n, 128].  The cube (utils.py:351-379, :325-348) is never materialised: the first-block
        kernel gathers its patches from the feature rows.  `timed(name, fn)`: the pipeline's HIP-event hook around each
        kernel (bench.py).
        Crop starts [n, K, 20]: K cubes of every clip, read from the clip's one set of rows (svk_c3d2_stage1_multi) ->
        [n, K, 128], each row what the [n, 20] call with crop_idx[:, k] gives; with pool="mean" (the float64 mean of a clip's K
        embeddings) or "mean_l2" (of its L2-normalised embeddings) -> [n, 128] (svk_embedding_pool)."""
        run = timed or (lambda name, fn: fn())
        eng = self.eng
        if pool not in (None, "mean", "mean_l2"):
            raise ValueError("pool must be None, 'mean' or 'mean_l2', got %r" % (pool,))
        if getattr(crop_idx, "ndim", 2) == 3:
            K = int(crop_idx.shape[1])
            if K < 1:
                raise ValueError("crop starts [n, K, 20] need K >= 1")
            emb = self._embed_multi(feat, crop_idx, run)
            if pool is None:
                return emb.view(-1, K, EMBED_DIM)
            return run("pool", lambda: eng.embedding_pool(emb, rows_per_seg=K, l2_rows=pool == "mean_l2"))
        self._check_rows(feat)
        return self._network(run, lambda: eng.c3d2_stage1(feat, crop_idx, self.stage1_tables(), live_cols=17))

    def _check_rows(self, feat):
        want = 3 if self.num_channels == 1 else 4
        if feat.dim() != want or (want == 4 and feat.shape[1] != self.num_channels):
            raise ValueError("this %d-channel model embeds feature rows of shape %s, got %s"
                             % (self.num_channels, "[n, T, 40]" if want == 3 else "[n, 3, T, 40]", tuple(feat.shape)))

    def _embed_multi(self, feat, crop_idx, run):
        """[n, K, 20] crop starts -> [n K, 128], cube-major: the first block reads clip u / K for cube u, the other six kernels
        see n K independent cubes."""
        self._check_rows(feat)
        return self._network(run, lambda: self.eng.c3d2_stage1(feat, crop_idx, self.stage1_tables(), cubes_per_clip=int(crop_idx.shape[1]),
                                                               live_cols=17))

    def _network(self, run, stage1):
        """The seven kernels behind `stage1()`, each through the timing hook.  The first block's output goes to the second block
        and nowhere else, so the callers ask for its 17 live columns (Engine.c3d2_stage1)."""
        eng = self.eng
        y = run("stage1", stage1)
        z = run("stage2", lambda: eng.c3d2_stage2(y, self.stage2_tables()))
        y = run("conv3_1", lambda: eng.c3d2_conv31(z, self.conv31_tables()))
        y = run("conv3_2", lambda: eng.c3d2_conv32t(y, self.conv32t_tables()))
        y = run("conv4_1", lambda: eng.c3d2_conv41(y, self.conv41_tables()))
        y = run("conv4_2", lambda: eng.c3d2_conv42(y, self.conv42_tables()))
        return run("fc5", lambda: eng.c3d2_fc5(y, self.fc5_tables()))

    @torch.no_grad()
    def __call__(self, cubes, batch=4096):
        """cubes [n, C, 20, 80, 40] f32 on the device (C = the model's 1 or 3 channels) -> [n, 128]: the cube's memory is read
        as [n, 1 600, 40] (or [n, 3, 1 600, 40]) feature rows with crop starts 0, 80, ... (a view: nothing is copied or
        re-gathered)."""
        shape = (self.num_channels,) + CUBE_SHAPE[1:]
        if cubes.dim() != 5 or tuple(cubes.shape[1:]) != shape:
            raise ValueError("expected cubes of shape (n, %d, 20, 80, 40), got %s" % (self.num_channels, tuple(cubes.shape)))
        x = self.eng.to_device(cubes, torch.float32)
        n = x.shape[0]
        if n:       # (this per-call surface only: the batched pipeline feeds its own features; aminmax: no temporary, NaN propagates)
            lo, hi = (float(v) for v in torch.aminmax(x))
        if n and not (lo > -65504.0 and hi < 65504.0):
            raise ValueError("cube values must be finite and below 65 504 in magnitude (the half-pair kernels' domain, include/svk.h); "
                             "the reference's features are log energies / MFCCs within +-100")
        rows = x.view((n,) + ((self.num_channels,) if self.num_channels != 1 else ()) + (CUBE_SHAPE[1] * CUBE_SHAPE[2], CUBE_SHAPE[3]))
        if n <= batch:
            return self.embed_features(rows, self.crop_starts(n, x.device)) if n else x.new_empty((0, EMBED_DIM))
        out = torch.empty((n, EMBED_DIM), dtype=torch.float32, device=x.device)
        for lo in range(0, n, batch):
            hi = min(n, lo + batch)
            out[lo:hi] = self.embed_features(rows[lo:hi], self.crop_starts(hi - lo, x.device))
        return out

    # ---- the operand tables of the seven entry points, built once in __init__ (layouts: the builders below) --------------
    def stage1_tables(self):
        return self._tables["stage1"]

    def stage2_tables(self):
        return self._tables["stage2"]

    def conv31_tables(self):
        return self._tables["conv31"]

    def conv32t_tables(self):
        return self._tables["conv32t"]

    def conv41_tables(self):
        return self._tables["conv41"]

    def conv42_tables(self):
        return self._tables["conv42"]

    def fc5_tables(self):
        return self._tables["fc5"]


# Two-piece f16 products (include/svk.h): a weight w is H = f16(w), L = f16(w - H), laid out in the lane order of
# v_mfma_f32_16x16x32_f16's A operand: lane l holds output channel co = 16 nt + (l & 15) and K index 8 kk + e (kk = l >> 4) in its
# eight halves e.  Each builder gathers the f32 weights of every (block, lane, e) at once through an index grid, then splits them.
def _grid(dev, *sizes):
    """Index tensors over the axes of the given sizes, each of the full shape `sizes`."""
    return torch.meshgrid(*(torch.arange(n, device=dev) for n in sizes), indexing="ij")


def _halves(w):
    """Gathered f32 weights [..., 64 lanes, 8] -> f16 [..., 2: H | L, 64, 8]."""
    h = w.to(torch.float16)
    return torch.stack((h, (w - h.to(torch.float32)).to(torch.float16)), dim=-3)


def _prelu(sl, co):
    """A PReLU's slope per output channel, and whether every slope lies in [0, 1] (the two-instruction form; one host read)."""
    return (sl.expand(co).contiguous() if sl.numel() == 1 else sl.contiguous()), bool(((sl >= 0) & (sl <= 1)).all())


def _stage1_tables(st1, st2):
    """Operand blocks of `svk_c3d2_stage1` / `svk_c3d2_stage1_c3` (conv1_1 1 or 3 -> 16 k(3,1,5); conv1_2 16 -> 16 k(3,9,1) stride
    (1,2,1); pool), two-piece f16 products:
      w1blk [2][64][8]      : conv1_1, tap t = 8 (kk & 1) + e (t = 5 kd + kw; 15 -> 0): H for every kk | L for kk < 2, 0 above
             [3][2][64][8]  : the three-channel conv1_1 (`svk_c3d2_stage1_c3`): that block for each input channel -- the 45
                              taps padded to 48, tap 15 of every channel the zero pad
      w2blk [14][2][64][8]  : conv1_2, tap pairs (a | b): ci = 8 (kk & 1) + e at tap a (kk < 2) / b (kk >= 2); H | L;
                              pair 13 is tap (2, 8) alone against an [h | l] fragment: H at every kk | L for kk < 2, 0 above
    -> (w1blk, bias1, slope1, w2blk, bias2, slope2, every slope in [0, 1])."""
    (w1, b1, s1, *_), (w2, b2, s2, *_) = st1, st2
    dev = w1.device
    w1t = torch.cat([w1.reshape(16, -1, 15), torch.zeros((16, w1.shape[1], 1), device=dev)], 2)      # [co][ch][t], t = 15: zero
    ch, l, e = _grid(dev, w1.shape[1], 64, 8)
    w1blk = _halves(w1t[l & 15, ch, 8 * ((l >> 4) & 1) + e])                                          # [ch][2][64][8]
    w1blk[..., 1, 32:, :] = 0           # lanes kk >= 2 meet the h half of the patch only: no L there
    # conv1_2's tap pairs: taps (kd, kh) a for kk < 2 | b for kk >= 2; pair 13's b is its a (the lone tap: H at every kk)
    pairs = torch.tensor([((p // 4, 2 * (p % 4)), (p // 4, 2 * (p % 4) + 1)) for p in range(12)]
                         + [((0, 8), (1, 8)), ((2, 8), (2, 8))], device=dev)                          # [14][a | b][kd, kh]
    p, l, e = _grid(dev, 14, 64, 8)
    tap = pairs[p, (l >> 5)]
    w2blk = _halves(w2[l & 15, 8 * ((l >> 4) & 1) + e, tap[..., 0], tap[..., 1], 0])                  # [14][2][64][8]
    w2blk[13, 1, 32:, :] = 0            # the lone tap is read as [h | l]: L against the h half only
    slope1, in01_1 = _prelu(s1, 16)
    slope2, in01_2 = _prelu(s2, 16)
    return (w1blk[0] if w1.shape[1] == 1 else w1blk, b1, slope1, w2blk, b2, slope2, in01_1 and in01_2)


def _stage2_tables(st1, st2):
    """Operand blocks of `svk_c3d2_stage2` (conv2_1 16 -> 32 k(3,1,4); conv2_2 32 -> 32 k(3,8,1) stride (1,2,1) + pool), two-piece
    f16 products:
      w21blk [2 nt][6 pairs][2][64][8]: conv2_1, pair = 2 kd + kw / 2: element e = W[co][ci = 8 (kk & 1) + e][kd][kw + (kk >= 2)]
      w22blk [2 nt][24 taps][2][64][8]: conv2_2, tap = 8 kd + kh: element e = W[co][ci = 8 kk + e][kd][kh] (K = 32 = one tap)
    -> (w21blk, bias21, slope21, w22blk, bias22, slope22, every slope in [0, 1])."""
    (w1, b1, s1, *_), (w2, b2, s2, *_) = st1, st2
    nt, pr, l, e = _grid(w1.device, 2, 6, 64, 8)
    kk = l >> 4
    w21blk = _halves(w1[16 * nt + (l & 15), 8 * (kk & 1) + e, pr // 2, 0, 2 * (pr % 2) + (kk >= 2).long()])
    nt, tap, l, e = _grid(w2.device, 2, 24, 64, 8)
    w22blk = _halves(w2[16 * nt + (l & 15), 8 * (l >> 4) + e, tap // 8, tap % 8, 0])
    slope1, in01_1 = _prelu(s1, 32)
    slope2, in01_2 = _prelu(s2, 32)
    return (w21blk, b1, slope1, w22blk, b2, slope2, in01_1 and in01_2)


def _conv31_tables(st):
    """`svk_c3d2_conv31` (conv3_1: 32 -> 64, k(3,1,3)), two-piece f16 products: wblk [4 nt][9 taps][2: H | L][64][8], element
    e = W[co][8 kk + e][kd][kw], tap 3 kd + kw -> (wblk, bias, slope [64], every slope in [0, 1])."""
    w, b, sl, *_ = st
    nt, tap, l, e = _grid(w.device, 4, 9, 64, 8)
    return (_halves(w[16 * nt + (l & 15), 8 * (l >> 4) + e, tap // 3, 0, tap % 3]), b) + _prelu(sl, 64)


def _conv32t_tables(st):
    """`svk_c3d2_conv32t` (conv3_2: 64 -> 64, k(3,7,1)), two-piece f16 products: wblk [4 nt][2 kb][21 taps][2: H | L][64][8],
    element e = W[co][32 kb + 8 kk + e][kd][kh], tap 7 kd + kh -> (wblk, bias, slope [64], every slope in [0, 1])."""
    w, b, sl, *_ = st
    nt, kb, tap, l, e = _grid(w.device, 4, 2, 21, 64, 8)
    return (_halves(w[16 * nt + (l & 15), 32 * kb + 8 * (l >> 4) + e, tap // 7, tap % 7, 0]), b) + _prelu(sl, 64)


def _conv41_tables(st):
    """`svk_c3d2_conv41` (conv4_1: 64 -> 128, k(3,1,3)), two-piece f16 products: wblk [8 nt][9 taps][2 kb][2: H | L][64][8],
    element e = W[co][32 kb + 8 kk + e][kd][kw], tap 3 kd + kw -> (wblk, bias, slope [128], every slope in [0, 1])."""
    w, b, sl, *_ = st
    nt, tap, kb, l, e = _grid(w.device, 8, 9, 2, 64, 8)
    return (_halves(w[16 * nt + (l & 15), 32 * kb + 8 * (l >> 4) + e, tap // 3, 0, tap % 3]), b) + _prelu(sl, 128)


def _conv42_tables(st):
    """`svk_c3d2_conv42` (conv4_2: 128 -> 128, k(3,7,1)), f32 through Winograd F(2, 3) along depth: the BN-folded weight g is
    transformed to G0 = g0, G1 = ((g0 + g2) + g1) / 2, G2 = ((g0 + g2) - g1) / 2, G3 = g2 (the expressions the kernel's prologue
    evaluates) and laid out as wfrag [8 nt][16 chunks of 8 input channels][7 taps][4 k][64 lanes][2]: lane (co = 16 nt + (l & 15),
    kk = l >> 4), element e = G_k[co][8 chunk + 2 kk + e][tap] -> (wfrag, bias, slope [128], every slope in [0, 1])."""
    w, b, sl, *_ = st
    g0, g1, g2 = w[:, :, 0, :, 0], w[:, :, 1, :, 0], w[:, :, 2, :, 0]                               # [co][ci][kh]
    g = torch.stack((g0, 0.5 * ((g0 + g2) + g1), 0.5 * ((g0 + g2) - g1), g2))                         # [4 k][co][ci][taps]
    lane = torch.arange(64, device=w.device)
    gg = g.view(4, 8, 16, 16, 4, 2, 7)                                                                # [k][nt][n][chunk][kq][e][tap]
    frag = gg[:, :, lane & 15, :, lane >> 4].permute(2, 3, 5, 1, 0, 4).contiguous()                   # lane axis first -> [nt][chunk][tap][k][lane][e]
    return (frag, b) + _prelu(sl, 128)


def _fc5_tables(fc_w, fc_b):
    """`svk_c3d2_fc5`: wfrag [4 d][8 nt][72 steps][64 lanes][4]: lane (j = 16 nt + (l & 15), kk = l >> 4), e:
    W5[j][c * 36 + d * 9 + pixel] for the K index 1 152 d + 16 step + 4 kk + e = ((d * 16 + chunk) * 9 + pixel) * 8 + c % 8
    (conv4_2's chunked output order; model.py:168 flattens NCDHW) -> (wfrag, bias)."""
    dev = fc_w.device
    # columns of the chunked order: [d][chunk][pixel][c8] -> torch column (8 chunk + c8) * 36 + d * 9 + pixel
    d, ch, px, c8 = _grid(dev, 4, 16, 9, 8)
    col = ((8 * ch + c8) * 36 + d * 9 + px).reshape(-1)                  # [4608] in K order
    lane = torch.arange(64, device=dev)
    wv = fc_w[:, col].view(8, 16, 4, 72, 4, 4)                           # [nt][n][d][step][kq][e]
    frag = wv[:, lane & 15, :, :, lane >> 4].permute(2, 1, 3, 0, 4).contiguous()   # lane axis first -> [d][nt][step][lane][e]
    return frag, fc_b.contiguous()


def seeded_model(seed, n_labels=1211, num_channels=1):
    """Random-init C3D2 under a fixed torch seed (the reference's checkpoint
    `Models/model_14_percent_best_so_far.pt` does not ship)."""
    gen_state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    model = C3D2(n_labels, num_channels)
    torch.random.set_rng_state(gen_state)
    return model.eval()


def calibrate_batchnorm(model, cubes, batch=64):
    """Set every BatchNorm3d's running statistics to the statistics of `cubes` (cumulative
    average over batches), as a trained network's would be.  A fresh random-init C3D2 has
    running mean 0 / var 1 while its activations are far from that, which makes the 128-d
    output almost input-independent (all cosine scores within 1e-3 of 1.0) and the EER a coin
    flip decided by rounding noise; calibrated statistics give a well-conditioned, still
    untrained, embedding.  Deterministic given the weights and `cubes`."""
    norms = [m for m in model.modules() if isinstance(m, nn.BatchNorm3d)]
    saved = [(m.momentum, m.training) for m in norms]
    was_training = model.training
    for m in norms:
        m.reset_running_stats()
        m.momentum = None                      # cumulative moving average
    model.train()
    with torch.no_grad():
        for lo in range(0, cubes.shape[0], batch):
            model(cubes[lo:lo + batch], development=False)
    for m, (momentum, _) in zip(norms, saved):
        m.momentum = momentum
    model.train(was_training)
    return model


def perturb_inference_state(state_dict, seed):
    """Give BatchNorm running statistics, affine terms and PReLU slopes
    non-trivial values (a fresh init has mean 0 / var 1 / slope 0.25, which
    would leave BN folding and PReLU untested).  In place, deterministic."""
    gen = torch.Generator().manual_seed(seed)
    for key in sorted(state_dict.keys()):
        t = state_dict[key]
        if key.endswith("running_mean"):
            t.copy_(0.05 * torch.randn(t.shape, generator=gen))
        elif key.endswith("running_var"):
            t.copy_(0.5 + torch.rand(t.shape, generator=gen))
        elif "batch_norm" in key and key.endswith(".weight"):
            t.copy_(0.8 + 0.4 * torch.rand(t.shape, generator=gen))
        elif "batch_norm" in key and key.endswith(".bias"):
            t.copy_(0.05 * torch.randn(t.shape, generator=gen))
        elif "PReLu" in key:
            t.copy_(0.1 + 0.3 * torch.rand(t.shape, generator=gen))
    return state_dict


def _enrolled(emb, speaker_ids, enroll):
    """{speaker id: (1, 128) CPU tensor} from utterance embeddings [n, 128] (device or host) and their ids: enroll="last" keeps
    each speaker's LAST listed utterance (the reference, Q17), "mean" the mean of the speaker's L2-normalised utterance
    embeddings (pipeline.enroll_mean: one svk_embedding_pool launch)."""
    if enroll not in ("last", "mean"):
        raise ValueError("enroll must be 'last' or 'mean', got %r" % (enroll,))
    ids = [str(v) for v in speaker_ids]
    if enroll == "mean":
        from .pipeline import enroll_mean
        uniq, models = enroll_mean(emb, ids, l2=True)
        models = models.cpu()
        first = {}
        for k, sid in enumerate(ids):           # the dict keeps the order in which speakers were first listed, as "last" does
            first.setdefault(sid, k)
        rows = {str(sid): models[k:k + 1].clone() for k, sid in enumerate(uniq)}
        return {sid: rows[sid] for sid in first}
    emb = emb.cpu()
    store = {}
    for i, sid in enumerate(ids):
        store[sid] = emb[i:i + 1].clone()
    return store


def _create_speaker_models_files(enroll="last"):
    """model.py:351-388 as written: checkpoint, enrolment list, id table and WAV tree under
    `constants.ROOT` / `constants.DATA_ORIGIN`; one `{speaker_id}.pt` (a (1, 128) tensor) per
    speaker under ROOT/speaker_models, the LAST listed utterance winning (Q17) -- or, with enroll="mean", the speaker's mean."""
    import os
    from . import constants as c
    from .evaluation import dataset_embeddings, load_indexed_labels
    from .utils import create_dataset
    model_path = os.path.join(c.ROOT, 'Models/model_14_percent_best_so_far.pt')
    save_speaker_models_path = os.path.join(c.ROOT, 'speaker_models')
    enrollment_set = os.path.join(c.ROOT, '50_first_ids.txt')
    indexed_labels = load_indexed_labels(c.ROOT + '/50_first_ids.npy')
    dataset = create_dataset(indexed_labels=indexed_labels, origin_file_path=enrollment_set)
    if not os.path.exists(save_speaker_models_path):
        os.mkdir(save_speaker_models_path)
    model = C3D2(100, 1).load_checkpoint(torch.load(model_path, map_location="cpu", weights_only=True))
    store = _enrolled(dataset_embeddings(dataset, model), [f[0:7] for f in dataset.sound_files], enroll)
    for sid, vec in store.items():
        torch.save(vec, '{}/{}.pt'.format(save_speaker_models_path, sid))
    return store


def create_speaker_models(model=None, cubes=None, speaker_ids=None, save_dir=None, batch=256, enroll="last"):
    """Enrolment as `/root/reference/model.py:351-388` does it.  With no arguments: file-driven, the
    paths of `constants` (see `_create_speaker_models_files`).  With `(model, cubes, speaker_ids)`: the
    same on in-memory cubes.  Every utterance cube is embedded
    with `development=False`; the speaker model is the embedding of that speaker's LAST listed
    utterance -- the reference overwrites `{speaker_id}.pt` on each utterance, no averaging
    (Q17).  Returns `{speaker_id: (1, 128) CPU tensor}` and, with `save_dir`, writes the
    reference's `{speaker_id}.pt` files (readable by `evaluation.Evaluation`).
    enroll="mean": the speaker model is the mean of the speaker's L2-normalised utterance embeddings instead
    (`pipeline.enroll_mean`, on the device); the default "last" is the reference's behaviour, unchanged."""
    import os
    if enroll not in ("last", "mean"):
        raise ValueError("enroll must be 'last' or 'mean', got %r" % (enroll,))
    if model is None and cubes is None:
        return _create_speaker_models_files(enroll)
    device = next(model.parameters()).device
    model.eval()
    store, rows = {}, []
    with torch.no_grad():
        for lo in range(0, len(cubes), batch):
            x = torch.as_tensor(cubes[lo:lo + batch], dtype=torch.float32).to(device)
            if enroll == "mean":
                rows.append(model(x, development=False))
                continue
            emb = model(x, development=False).cpu()
            for k in range(emb.shape[0]):
                store[str(speaker_ids[lo + k])] = emb[k:k + 1].clone()
    if enroll == "mean":
        store = _enrolled(torch.cat(rows), speaker_ids[:len(cubes)], "mean") if rows else {}
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        for sid, vec in store.items():
            torch.save(vec, os.path.join(save_dir, f"{sid}.pt"))
    return store
