"""Float64 references, the float32 yardstick and the bars for the stage kernels (csrc/stages.hip: svk_preemphasis,
svk_stack_frames, svk_spectrum, svk_mel_features) -- TEST INFRASTRUCTURE.

The float64 restatements follow oracle/speechpy_ref.py (and through it the reference's processing.py / feature.py; the
lines are cited per function) with the points the C entry points make explicit: the pre-emphasis shift is reduced mod n,
the coefficient is the float32 value the ABI carries, framing takes (frame_len, stride, n_frames) in samples and pads
with zeros past the signal, a frame longer than nfft is cut, and the mel stage starts from a power spectrum and a bank
that are float32 arrays (widened exactly).  Every restatement takes a `mutant` name: the planted faults the bars must
catch (MUTANTS lists them per stage).

Bars (u = 2^-24, the float32 unit roundoff):
  pre-emphasis   derived: the kernel rounds c * x_j and the difference, or fuses them:
                 |got - ref| <= 1.01 u (|c x_j| + |ref|).
  framing        bit-exact against the NumPy float32 expression (`frames32`).
  direct DFT     derived: float64 accumulators, twiddles rounded once to float32 (each component within 2^-25), one final
                 rounding: |X^_k - X_k| <= 1.01 (sqrt(2) 2^-25 ||x||_1 + u |X_k|).
  the FFT paths  measured like the fused front end's: the yardstick is torch.fft.rfft on the float32 frames and a float32
                 abs; errors are amplitudes divided by the frame's ||x||_2 (at nfft 512: by the larger ||x||_2 of the two
                 frames that share a transform); with y the yardstick's worst normalised error over the batch the kernel
                 passes when its own worst is at most K max(y, 2^-23), K = 4.  `margin512` is the one way K rises: a
                 float32 emulation of the packed path's own order of operations exceeds 4 on the same input -> twice its
                 ratio, at most 16.
  power          from the amplitude bar d of the same frame and bin, no second constant:
                 |p^ - p| <= (2 |X_k| d + d^2) / nfft + 4 u p.
  zeros          a frame of zeros gives zeros bit for bit on every path and both outputs.
  mel stage      derived: a float32 dot product of nbins terms in any order: |m^ - m| <= (nbins + 1) u sum |p_k| |b_k|;
                 frame energy nbins u sum |p_k|; log outputs: the relative bar + 2 ulp32 of the logarithm; cepstrum c:
                 sum_n |d_cn| bar(lm_n) + (nf / 2 + 3) u sum_n |lm_n| |d_cn| (two fma chains, the table's one rounding).
                 Where the float64 value is exactly 0 the linear output is float32(2^-52) bit for bit and the logarithm
                 within 1 ulp32 of float32(log 2^-52).  An element may be left out only where the float64 mel energy lies
                 strictly between 0 and 1e-30 (a float32 underflow could turn it into eps); `mel_judge` counts them.
"""
import numpy as np

from oracle import speechpy_ref as sp

K = 4
U = 2.0 ** -24
FLOOR = 2.0 ** -23
EPS64 = float(np.finfo(np.float64).eps)            # 2^-52 (functions.py:55-62)
EPS32 = np.float32(EPS64)
LOG_EPS32 = np.float32(np.log(EPS64))
UNDERFLOW = 1e-30
MFE, LMFE, MFCC = 0, 1, 2

MUTANTS = {
    "preemph": ("shift_sign",),
    "frames": ("pad_last", "window_shift"),
    "spectrum": ("wrap", "fold", "div_flen", "no_nyquist", "bin_mirror", "pair_swap", "silent_leak"),
    "mel": ("energy_64_bins", "no_eps", "dct_row0", "c0_replaced", "filter_last_bin"),
}


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- pre-emphasis (processing.py:45-58; oracle.speechpy_ref.preemphasis) ------------------------------------------------
def preemphasis(x, shift=1, cof=0.98, mutant=None, cof32=True):
    """y[i] = x[i] - c x[(i - shift) mod n] in float64 -> (y, |c x_j|).  c = float32(cof), the value svk_preemphasis
    receives (cof32 = False: the Python float, as the reference has it)."""
    x = np.asarray(x).astype(np.float64)
    n = x.size
    s = int(shift) if mutant != "shift_sign" else -int(shift)
    j = (np.arange(n, dtype=np.int64) - s) % n
    cx = (float(np.float32(cof)) if cof32 else float(cof)) * x[j]
    return x - cx, np.abs(cx)


def preemph_bar(y, cx):
    return 1.01 * U * (cx + np.abs(y))


# ---- framing (processing.py:61-139; oracle.speechpy_ref.stack_frames) ------------------------------------------------
def frames(sig, flen, stride, T, window=None, mutant=None, dtype=np.float64):
    """[T, flen]: sig[t stride + j], 0 past the signal's end (processing.py:107-109), times window[j] (:137-138).
    dtype = float32 gives the expression the kernel must equal bit for bit (one float32 multiply)."""
    sig = np.asarray(sig).astype(dtype)
    idx = np.arange(T, dtype=np.int64)[:, None] * stride + np.arange(flen, dtype=np.int64)[None, :]
    inside = idx < sig.size
    out = np.where(inside, sig[np.minimum(idx, max(sig.size - 1, 0))] if sig.size else 0, 0).astype(dtype)
    if mutant == "pad_last" and sig.size:
        out = np.where(inside, out, sig[-1]).astype(dtype)
    if window is not None:
        w = np.asarray(window).astype(dtype)
        if mutant == "window_shift":
            w = np.roll(w, 1)
        out = (out * w[None, :]).astype(dtype)
    return out


def frames32(sig, flen, stride, T, window=None):
    return frames(sig, flen, stride, T, window, dtype=np.float32)


# ---- spectrum (processing.py:142-174; oracle.speechpy_ref.fft_spectrum / power_spectrum) -------------------------------
def seen(fr, nfft):
    """The min(frame_len, nfft) samples of each frame the transform sees, float64."""
    return np.asarray(fr).astype(np.float64)[:, :nfft]


def spectrum(fr, nfft, mutant=None):
    """(|rfft(frame[:nfft], n = nfft)|, |.|^2 / nfft) in float64, [T, nfft/2 + 1] each."""
    fr = np.asarray(fr).astype(np.float64)
    T, flen = fr.shape
    x = np.zeros((T, nfft))
    x[:, :min(flen, nfft)] = fr[:, :nfft]
    if mutant == "wrap" and flen < nfft:               # the frame repeats where zeros belong
        x = fr[:, np.arange(nfft) % flen]
    if mutant == "fold" and flen > nfft:               # a long frame folded onto itself, not cut
        for s in range(nfft, flen, nfft):
            part = fr[:, s:s + nfft]
            x[:, :part.shape[1]] += part
    full = np.fft.fft(x, axis=-1)
    k = np.arange(nfft // 2 + 1)
    if mutant == "bin_mirror":                         # bin k read from nfft - k + 1
        k = (nfft - k + 1) % nfft
    amp = np.abs(full[:, k])
    if mutant == "no_nyquist" and nfft % 2 == 0:
        amp[:, -1] = 0.0
    power = amp * amp / (flen if mutant == "div_flen" else nfft)
    if mutant == "pair_swap":
        for i in range(0, T - 1, 2):
            amp[[i, i + 1]] = amp[[i + 1, i]]
            power[[i, i + 1]] = power[[i + 1, i]]
    if mutant == "silent_leak":                        # a silent frame inherits 1e-14 of its partner's power
        for i in range(0, T - 1, 2):
            for a, b in ((i, i + 1), (i + 1, i)):
                if not x[a].any() and x[b].any():
                    power[a] = 1e-14 * power[b]
                    amp[a] = np.sqrt(power[a] * nfft)
    return amp, power


def yardstick32(fr, nfft):
    """torch.fft.rfft on the float32 frames, float32 abs: it knows nothing of the kernels."""
    import torch
    x = np.array(np.asarray(fr, dtype=np.float32)[:, :nfft], order="C")         # a writable copy
    return torch.fft.rfft(torch.from_numpy(x), n=nfft, dim=-1).abs().numpy()


def pair_norms(x):
    """||x||_2 per frame, raised to the partner's (frames 2i, 2i + 1; an odd batch's last frame stands alone)."""
    n = np.sqrt((x * x).sum(axis=1))
    out = n.copy()
    m = (len(n) // 2) * 2
    both = np.maximum(n[0:m:2], n[1:m:2])
    out[0:m:2] = both
    out[1:m:2] = both
    return out


def emulation_packed512(fr):
    """Amplitudes the way spectrum_fft_kernel<false> orders its arithmetic, in float32 NumPy / torch-CPU: frames 2i and
    2i + 1 (a lone last frame with zeros) are the real and imaginary part of ONE 512-point complex64 transform, untangled
    as 2 X1 = Z[k] + conj Z[N-k], 2i X2 = Z[k] - conj Z[N-k]; |.|^2 x 1/4, square root; a silent frame's bins are 0."""
    import torch
    f32 = np.float32
    fr = np.asarray(fr, dtype=f32)
    T = fr.shape[0]
    x = np.zeros((T + (T & 1), 512), dtype=f32)
    x[:T, :min(fr.shape[1], 512)] = fr[:, :512]
    a, b = x[0::2], x[1::2]
    z = torch.fft.fft(torch.complex(torch.from_numpy(a.copy()), torch.from_numpy(b.copy())), dim=-1).numpy()
    k = np.arange(257)
    zk, zn = z[:, k], np.conj(z[:, (512 - k) % 512])
    xa, xb = (zk + zn).astype(np.complex64), (zk - zn).astype(np.complex64)
    pa = np.sqrt(((xa.real * xa.real + xa.imag * xa.imag) * f32(0.25)).astype(f32))
    pb = np.sqrt(((xb.real * xb.real + xb.imag * xb.imag) * f32(0.25)).astype(f32))
    pa[~a.any(axis=1)] = 0
    pb[~b.any(axis=1)] = 0
    out = np.zeros((T + (T & 1), 257), dtype=f32)
    out[0::2], out[1::2] = pa, pb
    return out[:T]


def fft_judge(got, fr, nfft, power, pair, margin=K, ref=None):
    """One launch of an FFT path.  got [T, nbins] (amplitude, or power when `power`); pair: nfft-512 packing.
    -> dict(ok, ratio, y, zeros_ok, why).  ratio: amplitude -- worst normalised error / max(y, 2^-23), passes when
    <= margin; power -- worst |p^ - p| / bound, passes when <= 1.  A frame of zeros must come back as exact zeros."""
    x = seen(fr, nfft)
    amp, pw = ref if ref is not None else spectrum(fr, nfft)
    norm = pair_norms(x) if pair else np.sqrt((x * x).sum(axis=1))
    live = norm > 0
    nrm = np.where(live, norm, 1.0)[:, None]
    y32 = yardstick32(fr, nfft).astype(np.float64)
    y = max(float((np.abs(y32 - amp) / nrm)[live].max()) if live.any() else 0.0, FLOOR)
    got = np.asarray(got, dtype=np.float64)
    silent = ~x.any(axis=1)
    zeros_ok = bool((got[silent] == 0).all())
    finite = bool(np.isfinite(got).all())
    if not power:
        ratio = float((np.abs(got - amp) / nrm)[live].max() / y) if live.any() else 0.0
        ok = finite and zeros_ok and ratio <= margin
    else:
        d = margin * y * norm[:, None]
        bound = (2.0 * amp * d + d * d) / nfft + 4.0 * U * pw
        err = np.abs(got - pw)
        ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
        ok = finite and zeros_ok and bool((err <= bound).all())
    why = "" if ok else "ratio %.3g (margin %g, yardstick %.3g), silent frames exact: %s" % (ratio, margin, y, zeros_ok)
    return dict(ok=ok, ratio=ratio, y=y, zeros_ok=zeros_ok, why=why)


def margin512(fr):
    """The margin of an nfft-512 launch: K, unless the float32 emulation of the packed path exceeds K on this very input;
    then twice the emulation's ratio and never past 16.  -> (margin, the emulation's ratio)"""
    r = fft_judge(emulation_packed512(fr), fr, 512, False, True)["ratio"]
    return (min(16.0, 2.0 * r) if r > K else K), r


def dft_judge(got, fr, nfft, power, ref=None):
    """One launch of the direct DFT: the derived bar per bin.  -> dict(ok, ratio, zeros_ok, why); ratio = worst err / bar."""
    x = seen(fr, nfft)
    amp, pw = ref if ref is not None else spectrum(fr, nfft)
    d = 1.01 * (np.sqrt(2.0) * 2.0 ** -25 * np.abs(x).sum(axis=1)[:, None] + U * amp)
    got = np.asarray(got, dtype=np.float64)
    silent = ~x.any(axis=1)
    zeros_ok = bool((got[silent] == 0).all())
    want, bound = (pw, (2.0 * amp * d + d * d) / nfft + 4.0 * U * pw) if power else (amp, d)
    err = np.abs(got - want)
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    ok = bool(np.isfinite(got).all()) and zeros_ok and bool((err <= bound).all())
    return dict(ok=ok, ratio=ratio, zeros_ok=zeros_ok, why="" if ok else "worst error %.3g x the bar, silent frames exact: %s"
                % (ratio, zeros_ok))


# ---- mel / log / DCT stage (feature.py:102-153, :156-219; oracle.speechpy_ref.mfe / mfcc) -------------------------------
def mel(power, bank, num_ceps=13, mutant=None):
    """From a power spectrum [T, nbins] and a bank [nf, nbins] (float32 arrays, widened exactly) in float64:
    dict(mel, energy (both after zero_handling), mel_raw, energy_raw, logmel, ceps_dc, ceps_nodc, dct)."""
    p = np.asarray(power).astype(np.float64)
    b = np.asarray(bank).astype(np.float64).copy()
    nf = b.shape[0]
    if mutant == "filter_last_bin":
        b[-1, -1] = 0.0
    e_raw = (p[:, :64] if mutant == "energy_64_bins" else p).sum(axis=1)       # feature.py:202: ALL bins
    m_raw = p @ b.T                                                              # feature.py:213
    if mutant == "no_eps":
        m, e = m_raw, e_raw
    else:
        m, e = sp.zero_handling(m_raw), sp.zero_handling(e_raw)                  # feature.py:205, :217
    with np.errstate(divide="ignore", invalid="ignore"):
        lm, le = np.log(m), np.log(e)
    dct = sp.dct2_ortho_matrix(num_ceps, nf)                                     # feature.py:147
    if mutant == "dct_row0":
        dct[0, :] = np.sqrt(2.0 / nf)
    with np.errstate(invalid="ignore"):
        nodc = lm @ dct.T
    dc = nodc.copy()
    dc[:, 0] = le                                                                # feature.py:151-152
    if mutant == "c0_replaced":
        nodc = dc.copy()
    return dict(mel=m, energy=e, mel_raw=m_raw, energy_raw=e_raw, logmel=lm, ceps_dc=dc, ceps_nodc=nodc, dct=dct)


def mel_bars(power, bank, ref):
    """dict(mel, energy, logmel, logenergy, ceps): the derived bars, float64 arrays shaped like the outputs.  Where the
    raw float64 value is exactly 0 the linear bar is 0 (the output is float32(eps) bit for bit: `mel_judge` compares with
    that) and the log bar is 1 ulp32 of log eps."""
    p = np.abs(np.asarray(power).astype(np.float64))
    b = np.abs(np.asarray(bank).astype(np.float64))
    nbins = p.shape[1]
    nf = b.shape[0]
    bm = (nbins + 1) * U * (p @ b.T)
    be = nbins * U * p.sum(axis=1)

    def logbar(bar, raw, val):
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(raw == 0, 0.0, bar / np.abs(raw))
            lb = np.where(rel < 1, -np.log1p(-np.minimum(rel, 1.0 - 2.0 ** -30)), np.inf) + 2.0 * _ulp32(np.log(np.abs(val)))
        return np.where(raw == 0, _ulp32(LOG_EPS32), lb)

    blm = logbar(bm, ref["mel_raw"], ref["mel"])
    ble = logbar(be, ref["energy_raw"], ref["energy"])
    d = np.abs(ref["dct"])
    bc = blm @ d.T + (nf / 2.0 + 3.0) * U * (np.abs(ref["logmel"]) @ d.T)
    return dict(mel=bm, energy=be, logmel=blm, logenergy=ble, ceps=bc)


def mel_judge(got, energy, power, bank, out_kind, num_ceps, dc_elimination, ref=None, bars=None):
    """One launch of svk_mel_features.  got [T, cols]; energy [T] or None; ref / bars: `mel` and `mel_bars` of the same
    (power, bank), when the caller shares them between launches.
    -> dict(ok, ratio (worst error / bar), left_out (elements not compared), why)."""
    if ref is None:
        ref = mel(power, bank, num_ceps)
    if bars is None:
        bars = mel_bars(power, bank, ref)
    got = np.asarray(got)
    raw = ref["mel_raw"]
    under = (np.abs(raw) > 0) & (np.abs(raw) < UNDERFLOW)
    left = int(under.sum())
    worst, bad = 0.0, []

    def check(name, g, want, bar, exact=None, skip=None):
        nonlocal worst
        g64 = np.asarray(g, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            err = np.abs(g64 - want)
        err = np.where(np.isfinite(g64), err, np.inf)
        if skip is not None:
            err = np.where(skip, 0.0, err)
        if exact is not None:                          # (mask, float32 value): bit for bit
            mask, val = exact
            if not (np.asarray(g)[mask].astype(np.float32).view(np.int32) == np.float32(val).view(np.int32)).all():
                bad.append(name + ": eps substitution not exact")
            err = np.where(mask, 0.0, err)
            bar = np.where(mask, 1.0, bar)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bar)
        worst = max(worst, float(r.max()) if r.size else 0.0)
        if not (err <= bar).all():
            bad.append("%s: %.3g x the bar" % (name, float(r.max())))

    if out_kind == MFE:
        check("mfe", got, ref["mel"], bars["mel"], exact=(raw == 0, EPS32), skip=under)
    elif out_kind == LMFE:
        check("lmfe", got, ref["logmel"], bars["logmel"], skip=under)
    else:
        rows = under.any(axis=1)[:, None]
        want = (ref["ceps_dc"] if dc_elimination else ref["ceps_nodc"])[:, :num_ceps]
        bar = bars["ceps"][:, :num_ceps].copy()
        if dc_elimination:
            bar[:, 0] = bars["logenergy"]
        check("mfcc", got, want, bar, skip=np.broadcast_to(rows, want.shape))
    if energy is not None:
        check("energy", energy, ref["energy"], bars["energy"], exact=(ref["energy_raw"] == 0, EPS32))
    return dict(ok=not bad, ratio=worst, left_out=left, why="; ".join(bad))
