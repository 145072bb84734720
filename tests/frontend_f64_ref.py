"""Float64 reference, float32 yardstick and the bar for the fused front end (csrc/frontend.hip) -- TEST INFRASTRUCTURE.

`reference`      the whole chain PCM -> [pre-emphasis] -> frames -> |rfft|^2 / nfft -> frame energy -> mel -> log -> DCT-II
                 -> c0 := log E in float64 NumPy, for one clip.  It follows oracle/speechpy_ref.py with three points made
                 explicit: the signal is float64 BEFORE the pre-emphasis, the coefficient and input_scale are the float32
                 values svk_frontend_cfg carries (widened), and a frame longer than nfft is cut to nfft samples.
`restatement32`  the same chain in plain float32 (torch.fft.rfft on float32 CPU tensors, float32 products): the yardstick.
                 It knows nothing of the kernel's layout.  Its `mutant` argument plants the faults the bar must catch.
`compare`        the bar.  Per output column c (a filter, a cepstrum, the energy) y32[c] is the yardstick's worst error
                 over all valid frames of the batch -- relative for the linear outputs (MFE, energy), absolute for the
                 logarithmic ones -- and a result passes when its own worst error per column is at most
                 K * max(y32[c], floor[c]), floor = 2 float32 ulps of the column's largest reference magnitude (so a
                 lucky yardstick cannot set a bar of zero).  K = 4: on top of a plain float32 real FFT the kernel has one
                 more rounding stage (the untangling of two packed frames / of the even-odd halves), float32 twiddle and
                 bank tables, a frame energy from Parseval partial sums and products accumulated in the MFMA's order --
                 each on the order of one more unit of the same rounding, on a yardstick that already sits at a few units.
                 Frame counts are compared exactly.
`margin`         the one way the margin of a launch rises above K: an emulation of the path's own order of operations
                 (`emulation_packed512`, `emulation_dct_mfma`) exceeds K on the same input; then 2 x its ratio, at most 16.

An element may be left out only where the reference mel energy is below COND = 1e-9 of its frame's energy (the log of
such a value is not a meaningful comparison); `compare` reports the share, the tests assert it is 0 on their inputs.

`spec` is anything with the attributes of speaker_verification_amd.engine.FrontendSpec.
"""
import numpy as np

K = 4
COND = 1e-9
MFE, LMFE, MFCC = 0, 1, 2
EPS64 = float(np.finfo(np.float64).eps)


# ---- tables (float64) ---------------------------------------------------------------------------------------------
def mel_bank(spec):
    """(num_filters, nfft/2 + 1) triangular mel bank with SpeechPy's two quirks: a falsy low edge becomes 300 Hz, and
    the band edges map to bins with (nbins + 1) * hz / fs."""
    nbins = spec.nfft // 2 + 1
    high = spec.high_freq or spec.fs / 2
    low = spec.low_freq or 300
    mels = np.linspace(1127.0 * np.log(1.0 + low / 700.0), 1127.0 * np.log(1.0 + high / 700.0), spec.num_filters + 2)
    edges = np.floor((nbins + 1) * (700.0 * (np.exp(mels / 1127.0) - 1.0)) / spec.fs).astype(int)
    bank = np.zeros((spec.num_filters, nbins))
    for i in range(spec.num_filters):
        lo, mid, hi = int(edges[i]), int(edges[i + 1]), int(edges[i + 2])
        x = np.arange(lo, hi + 1, dtype=np.float64)
        y = np.zeros(x.shape)
        up = (x > lo) & (x <= mid)
        y[up] = (x[up] - lo) / (mid - lo)
        down = (x >= mid) & (x < hi)                   # runs second: x == mid takes the falling edge
        y[down] = (hi - x[down]) / (hi - mid)
        bank[i, lo:hi + 1] = y
    return bank


def dct_matrix(n_out, n_in):
    """First n_out rows of the orthonormal DCT-II of size n_in."""
    k = np.arange(n_out)[:, None]
    n = np.arange(n_in)[None, :]
    mat = np.sqrt(2.0 / n_in) * np.cos(np.pi * k * (2 * n + 1) / (2.0 * n_in))
    mat[0, :] = np.sqrt(1.0 / n_in)
    return mat


def num_frames(n_samples, spec):
    """(len - flen) // stride, 0 when len < flen: len == flen gives 0 frames."""
    return (n_samples - spec.frame_len) // spec.frame_stride if n_samples >= spec.frame_len else 0


def _num_ceps(spec):
    return max(1, min(spec.num_ceps, spec.num_filters))


def _frames(sig, T, spec):
    """[T, min(flen, nfft)]: a frame longer than nfft is cut, as rfft(n = nfft) does."""
    idx = np.arange(T)[:, None] * spec.frame_stride + np.arange(min(spec.frame_len, spec.nfft))[None, :]
    return sig[idx] if T > 0 else np.zeros((0, idx.shape[1]), dtype=sig.dtype)


# ---- float64 -----------------------------------------------------------------------------------------------------
def reference(pcm, spec):
    """One clip in float64 -> dict(n_frames, mel [T, F], energy [T], logmel [T, F], ceps_dc / ceps_nodc [T, num_ceps])."""
    x = np.asarray(pcm).astype(np.float64) * float(np.float32(spec.input_scale))
    if spec.preemph and x.size:
        x = x - float(np.float32(spec.preemph_cof)) * np.roll(x, spec.preemph_shift)
    T = num_frames(x.size, spec)
    spectrum = np.fft.rfft(_frames(x, T, spec), n=spec.nfft, axis=-1)
    power = (spectrum.real ** 2 + spectrum.imag ** 2) / spec.nfft
    energy = power.sum(axis=1)
    energy = np.where(energy == 0, EPS64, energy)
    mel = power @ mel_bank(spec).T
    mel = np.where(mel == 0, EPS64, mel)
    logmel = np.log(mel)
    nodc = logmel @ dct_matrix(_num_ceps(spec), spec.num_filters).T
    dc = nodc.copy()
    dc[:, 0] = np.log(energy)
    return dict(n_frames=T, mel=mel, energy=energy, logmel=logmel, ceps_dc=dc, ceps_nodc=nodc)


# ---- float32 -----------------------------------------------------------------------------------------------------
MUTANTS = ("no_wrap", "preemph_per_frame", "energy_no_nyquist", "energy_no_dc", "frame_more", "frame_fewer",
           "filter_last_bin", "bins_from_256", "dct_row0", "c0_kept", "c0_replaced", "fold", "scale_once")


def restatement32(pcm, spec, mutant=None):
    """One clip in plain float32; the same dict as `reference`, every array float32.

    mutant: None or one of MUTANTS --
      no_wrap            sample 0 of the pre-emphasis has no predecessor (no circular wrap)
      preemph_per_frame  the pre-emphasis restarts at each frame's first sample
      energy_no_nyquist  frame energy without bin nfft/2        energy_no_dc   without bin 0
      frame_more / frame_fewer   one frame too many / too few
      filter_last_bin    each filter loses its last non-zero bin
      bins_from_256      the bank's bins from 256 up are dropped
      dct_row0           DCT row 0 scaled by sqrt(2/N) like the others
      c0_kept            c0 not replaced by log E under dc_elimination;   c0_replaced   replaced when it is off
      fold               a frame longer than nfft is folded onto itself, not cut
      scale_once         input_scale reaches the energy once, not squared
    """
    import torch
    assert mutant is None or mutant in MUTANTS, mutant
    f32 = np.float32
    scale = f32(spec.input_scale)
    x = np.asarray(pcm).astype(f32) * scale
    n = x.size
    T = num_frames(n, spec)
    if mutant == "frame_more":
        T += 1 if n >= spec.frame_len else 0
    if mutant == "frame_fewer":
        T = max(T - 1, 0)
    cof = f32(spec.preemph_cof)
    if spec.preemph and n:
        prev = np.roll(x, spec.preemph_shift)
        if mutant == "no_wrap":
            prev[:spec.preemph_shift] = 0
        y = (x - cof * prev).astype(f32)
    else:
        y = x
    if mutant == "fold" and spec.frame_len > spec.nfft:
        idx = np.arange(T)[:, None] * spec.frame_stride + np.arange(spec.frame_len)[None, :]
        long = y[idx] if T > 0 else np.zeros((0, spec.frame_len), dtype=f32)
        frames = long[:, :spec.nfft].copy()
        frames[:, :spec.frame_len - spec.nfft] += long[:, spec.nfft:]
    else:
        frames = _frames(y, T, spec).copy()
    if mutant == "preemph_per_frame" and spec.preemph and T > 0:
        starts = np.arange(T) * spec.frame_stride
        for s in range(min(spec.preemph_shift, frames.shape[1])):
            frames[:, s] = x[starts + s]
    if T > 0:
        z = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(frames, dtype=f32)), n=spec.nfft, dim=-1)
        re, im = z.real.numpy(), z.imag.numpy()
    else:                                              # (an empty batch is not a transform the library plans)
        re = im = np.zeros((0, spec.nfft // 2 + 1), dtype=f32)
    power = ((re * re + im * im) * f32(1.0 / spec.nfft)).astype(f32)
    e_bins = power
    if mutant == "energy_no_nyquist":
        e_bins = power[:, :-1]
    if mutant == "energy_no_dc":
        e_bins = power[:, 1:]
    energy = e_bins.sum(axis=1, dtype=f32)
    if mutant == "scale_once" and scale != 0:
        energy = (energy / scale).astype(f32)
    energy = np.where(energy == 0, f32(EPS64), energy).astype(f32)
    bank = mel_bank(spec)
    if mutant == "filter_last_bin":
        for row in bank:
            nz = np.nonzero(row)[0]
            if nz.size:
                row[nz[-1]] = 0.0
    if mutant == "bins_from_256":
        bank[:, 256:] = 0.0
    mel = power @ bank.astype(f32).T
    mel = np.where(mel == 0, f32(EPS64), mel).astype(f32)
    logmel = np.log(mel).astype(f32)
    dct = dct_matrix(_num_ceps(spec), spec.num_filters)
    if mutant == "dct_row0":
        dct[0, :] = np.sqrt(2.0 / spec.num_filters)
    nodc = (logmel @ dct.astype(f32).T).astype(f32)
    dc = nodc.copy()
    dc[:, 0] = np.log(energy)
    if mutant == "c0_kept":
        dc = nodc.copy()
    if mutant == "c0_replaced":
        nodc = dc.copy()
    return dict(n_frames=T, mel=mel, energy=energy, logmel=logmel, ceps_dc=dc, ceps_nodc=nodc)


# ---- float32 emulation of the nfft-512 path's order of operations -------------------------------------------------
def emulation_packed512(pcm, spec, pack=True):
    """One clip the way frontend_kernel<.., SPLIT1024 = false, ..> orders its arithmetic, in float32 NumPy / torch-CPU:
    frames 2m and 2m + 1 of a clip (a lone last frame with zeros) are the real and the imaginary part of ONE 512-point
    complex transform; the two spectra are untangled as 2 X1 = Z[k] + conj Z[N-k], 2i X2 = Z[k] - conj Z[N-k]; the raw
    |.|^2 go to the bank product, whose float32 weights carry 1/nfft, the 1/4 of the untangling and input_scale^2; an
    all-zero frame's power bins are 0; the frame energy is Parseval's sum(x^2)/2 + (X[0]^2 + X[256]^2)/(2 nfft).
    The untangling separates the two frames only to the rounding of the LOUDER one: a quiet frame beside a loud one
    carries an error of about 2^-24 of its partner's amplitude, which no single-frame float32 transform has -- the one
    place where this path may exceed K times the yardstick (see `margin`).  pack=False gives every frame a transform of
    its own (a zero partner): the same arithmetic without the neighbour.  Same dict as `restatement32`."""
    import torch
    assert spec.nfft == 512
    f32 = np.float32
    x = np.asarray(pcm).astype(f32)
    T = num_frames(x.size, spec)
    if spec.preemph and x.size:
        x = (x - f32(spec.preemph_cof) * np.roll(x, spec.preemph_shift)).astype(f32)
    frames = np.zeros((T + (T & 1), 512), dtype=f32)
    frames[:T, :min(spec.frame_len, 512)] = _frames(x, T, spec)
    nbins, scale = 257, float(f32(spec.input_scale))
    power = np.zeros((T + (T & 1), nbins), dtype=f32)
    energy = np.zeros(T + (T & 1), dtype=f32)
    if T > 0:
        a, b = frames[0::2], frames[1::2]
        if not pack:
            a, b = frames, np.zeros_like(frames)
        z = torch.fft.fft(torch.complex(torch.from_numpy(a.copy()), torch.from_numpy(b.copy())), dim=-1).numpy()
        k = np.arange(nbins)
        zk, zn = z[:, k], np.conj(z[:, (512 - k) % 512])
        xa, xb = (zk + zn).astype(np.complex64), (zk - zn).astype(np.complex64)
        pa = (xa.real * xa.real + xa.imag * xa.imag).astype(f32)
        pb = (xb.real * xb.real + xb.imag * xb.imag).astype(f32)
        pa[~a.any(axis=1)] = 0
        pb[~b.any(axis=1)] = 0
        ends = lambda r: ((r[:, 0] * r[:, 0] + r[:, 256] * r[:, 256]) * f32(1.0 / 1024.0)).astype(f32)
        ea = f32(0.5) * (a * a).sum(axis=1, dtype=f32) + ends(z.real)
        eb = f32(0.5) * (b * b).sum(axis=1, dtype=f32) + ends(z.imag)
        if pack:
            power[0::2], power[1::2], energy[0::2], energy[1::2] = pa, pb, ea, eb
        else:
            power, energy = pa, ea
    power, energy = power[:T], (energy[:T] * f32(scale * scale)).astype(f32)
    energy = np.where(energy == 0, f32(EPS64), energy).astype(f32)
    weights = (mel_bank(spec) * (scale * scale / 2048.0)).astype(f32)
    mel = power @ weights.T
    mel = np.where(mel == 0, f32(EPS64), mel).astype(f32)
    logmel = np.log(mel).astype(f32)
    nodc = (logmel @ dct_matrix(_num_ceps(spec), spec.num_filters).astype(f32).T).astype(f32)
    dc = nodc.copy()
    dc[:, 0] = np.log(energy)
    return dict(n_frames=T, mel=mel, energy=energy, logmel=logmel, ceps_dc=dc, ceps_nodc=nodc)


def emulation_dct_mfma(mel, spec):
    """log and cepstra in the kernel's order, from float32 mel energies.  The logarithm is fast_log's: log2 rounded to
    float32 (v_log_f32), then times float32(ln 2), rounded again -- up to ~2 ulp where a float32 library log has 1/2.
    cepstra^T = DCT x log(mel)^T the way the kernel's v_mfma_f32_16x16x4_f32 chain accumulates it: float32 table, one
    float32 accumulator per cepstrum, the filters taken in the chain's order -- filter tile t, then register r, each
    instruction adding filters 16 t + r, + 4, + 8, + 12 -- every product added with one rounding.  A plain float32 matrix
    product splits the sum over SIMD lanes; this chain does not, and on log-mel vectors that are large and nearly
    constant (a very quiet float clip: log-mel around -63) the DCT's cosine rows run their partial sums up to ~200 before
    they cancel, so the chain's rounding is that of the partial sums, not of the result.  -> [T, num_ceps] float32."""
    f32 = np.float32
    nf = spec.num_filters
    table = dct_matrix(_num_ceps(spec), nf).astype(f32).astype(np.float64)
    log2 = np.log2(np.asarray(mel, dtype=f32).astype(np.float64)).astype(f32)
    x = (log2 * f32(np.log(2.0))).astype(f32).astype(np.float64)
    acc = np.zeros((x.shape[0], table.shape[0]), dtype=f32)
    for t in range((nf + 15) // 16):
        for r in range(4):
            for g in range(4):
                n = 16 * t + 4 * g + r
                if n < nf:
                    acc = (acc.astype(np.float64) + x[:, n:n + 1] * table[None, :, n]).astype(f32)
    return acc


def margin(clips, refs, yards, spec):
    """The bar's margin for one launch: K, except where a float32 emulation of the path's own order of operations exceeds K
    on this very input -- then twice the emulation's ratio, and never past 16.  Two paths have such an emulation:
      * the linear mel energies (MFE) of the nfft-512 path (`emulation_packed512`): two frames share a transform, and a
        relative error has no logarithm's floor under it;
      * the cepstra (`emulation_dct_mfma` on the yardstick's own mel energies): the two-instruction logarithm and the
        MFMA chain's accumulation order.
    -> (margin, the emulation's ratio or None)"""
    if spec.out_kind == MFE and spec.nfft == 512:
        gots = [as_result(emulation_packed512(x, spec), spec) for x in clips]
    elif spec.out_kind == MFCC:
        gots = []
        for y in yards:
            ceps = emulation_dct_mfma(y["mel"], spec)
            if spec.dc_elimination:
                ceps[:, 0] = y["ceps_dc"][:, 0]
            gots.append(dict(n_frames=y["n_frames"], feat=ceps, energy=y["energy"]))
    else:
        return K, None
    v = compare(gots, refs, yards, spec)
    worst = max(v["ratio_feat"], v["ratio_energy"])
    return (min(16.0, 2.0 * worst) if worst > K else K), worst


# ---- the bar -----------------------------------------------------------------------------------------------------
def output(res, spec):
    """The feature matrix a launch with `spec` returns, from a `reference` / `restatement32` dict."""
    if spec.out_kind == MFE:
        return res["mel"]
    if spec.out_kind == LMFE:
        return res["logmel"]
    return res["ceps_dc"] if spec.dc_elimination else res["ceps_nodc"]


def as_result(res, spec):
    """dict(n_frames, feat, energy): the form `compare` judges (what a launch returns for one clip, valid rows only)."""
    return dict(n_frames=res["n_frames"], feat=output(res, spec), energy=res["energy"])


def keep_mask(ref, spec):
    """Elements of the feature matrix that are compared: mel / frame energy >= COND (a frame's cepstra need all filters)."""
    ok = ref["mel"] >= COND * ref["energy"][:, None]
    if spec.out_kind == MFCC:
        return np.repeat(ok.all(axis=1)[:, None], _num_ceps(spec), axis=1)
    return ok


def _column_worst(gots, wants, keeps, linear):
    """Worst error per column over all clips (relative when `linear`), and the column's largest reference magnitude."""
    cols = wants[0].shape[1]
    err, mag = np.zeros(cols), np.zeros(cols)
    for got, want, keep in zip(gots, wants, keeps):
        if want.shape[0] == 0:
            continue
        d = np.abs(np.asarray(got, dtype=np.float64) - want)
        d = np.where(np.isfinite(d), d, np.inf)
        if linear:
            d = d / np.abs(want)
        err = np.maximum(err, np.where(keep, d, 0.0).max(axis=0))
        mag = np.maximum(mag, np.where(keep, np.abs(want), 0.0).max(axis=0))
    return err, mag


def _floor(mag, linear):
    """2 float32 ulps of the column's largest reference magnitude (as a relative error for the linear outputs)."""
    with np.errstate(over="ignore"):
        m32 = np.maximum(mag, np.finfo(np.float32).tiny).astype(np.float32)
    ulp = np.spacing(m32).astype(np.float64)
    return 2.0 * ulp / np.maximum(mag, np.finfo(np.float32).tiny) if linear else 2.0 * ulp


def compare(gots, refs, yards, spec, margin=K, energy=True):
    """Judge one launch.  gots / refs / yards: per clip, `as_result` dicts of the result under test (`max_frames` already
    applied: rows beyond it are absent), `reference` dicts and `restatement32` dicts.
    -> dict(ok, why, ratio_feat, ratio_energy, left_out): ratio_* is the worst error / max(y32, floor) over the columns,
    left_out the share of feature elements not compared."""
    out = dict(ok=True, why="", ratio_feat=0.0, ratio_energy=0.0, left_out=0.0)
    rows = []
    for i, (got, ref) in enumerate(zip(gots, refs)):
        if int(got["n_frames"]) != ref["n_frames"] or got["feat"].shape[0] != ref["n_frames"]:
            out.update(ok=False, why="clip %d: %d frames, want %d" % (i, int(got["n_frames"]), ref["n_frames"]))
            return out
        rows.append(ref["n_frames"])
    keeps = [keep_mask(ref, spec) for ref in refs]
    total = sum(k.size for k in keeps)
    out["left_out"] = float(sum(k.size - int(k.sum()) for k in keeps)) / max(total, 1)
    linear = spec.out_kind == MFE
    wants = [output(ref, spec) for ref in refs]
    y32, mag = _column_worst([output(y, spec) for y in yards], wants, keeps, linear)
    err, _ = _column_worst([g["feat"] for g in gots], wants, keeps, linear)
    bar = np.maximum(y32, _floor(mag, linear))
    out["ratio_feat"] = float((err / bar).max())
    if energy:
        wants_e = [ref["energy"][:, None] for ref in refs]
        all_e = [np.ones(w.shape, dtype=bool) for w in wants_e]
        y32e, mage = _column_worst([y["energy"][:, None] for y in yards], wants_e, all_e, True)
        erre, _ = _column_worst([np.asarray(g["energy"])[:, None] for g in gots], wants_e, all_e, True)
        out["ratio_energy"] = float((erre / np.maximum(y32e, _floor(mage, True))).max())
    worst = max(out["ratio_feat"], out["ratio_energy"])
    if not worst <= margin:
        out.update(ok=False, why="worst error %.2f x the yardstick (margin %g)" % (worst, margin))
    return out
