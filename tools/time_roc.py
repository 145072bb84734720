"""HIP-event medians of the device evaluation at dev-set scale (148 642 x 1 211 scores of seeded unit-norm embeddings, 128
dims, through svk_cosine_scores): svk_roc_eer, svk_roc_k (k = 1 and 10, with and without the curve), svk_top1, torch.sort of
the same scores (a yardstick), and evaluate(device=True) against device=False end to end on in-memory embeddings.  Next to
each time: the bytes the kernel moves by its design and the resulting TB/s against the 8 TB/s HBM peak.

SVK_TOOL_LIB=path/to/libsvk.so times another build (e.g. the parent commit's, under build_variants/); entry points that build
lacks are reported as missing.  SVK_ROC_SKIP_E2E=1 leaves out the end-to-end pair (the host path takes a minute).
One JSON line on stdout."""
import json
import os

import _timing as T          # (puts the repository on sys.path)

NT, NS, D = 148642, 1211, 128


def sort_bytes(n, passes):
    """The radix sort's traffic per its design: the histogram read (5 B per pair), then per pass the count read (4 B),
    the scatter's read (5 B) and write (5 B)."""
    return n * (5 + 14 * passes)


def main():
    import numpy as np
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd import evaluation
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    reps = int(os.environ.get("SVK_ROC_REPS", "10"))
    g = torch.Generator(device=eng.device).manual_seed(1)
    test = torch.nn.functional.normalize(torch.randn(NT, D, device=eng.device, generator=g), dim=1)
    enroll = torch.nn.functional.normalize(torch.randn(NS, D, device=eng.device, generator=g), dim=1)
    scores = eng.cosine_scores(test, enroll)
    true = torch.randint(0, NS, (NT,), device=eng.device, generator=g).to(torch.int32)
    labels = torch.zeros((NT, NS), dtype=torch.uint8, device=eng.device)
    labels[torch.arange(NT, device=eng.device), true.long()] = 1
    n = NT * NS
    sc, lb = scores.reshape(-1), labels.reshape(-1)
    res = T.header(_lib, lib, sha=False, n_pairs=n, ms={}, bytes={}, tb_s={})

    # passes the sort runs on these scores: a digit that is the same for every key is skipped
    keys = sc.view(torch.int32).cpu().numpy().view(np.uint32)
    keys = np.where(keys == 0x80000000, 0, keys)
    keys = ~np.where(keys & 0x80000000, ~keys, keys | 0x80000000)
    passes = sum(int(np.unique((keys >> (8 * p)) & 255).size > 1) for p in range(4)) or 1
    res["sort_passes"] = passes
    point_bytes = n * (5 + 5 + 8)        # (label, key) twice -- part and emit pass -- and the points written
    T.put("roc_eer", T.timed(torch, lambda: eng.roc_eer(sc, lb), reps), sort_bytes(n, passes) + point_bytes)
    if hasattr(lib, "svk_roc_k"):
        for k in (1, 10):
            for curve in (False, True):
                extra = n * 8 * 2 if curve else n * 8   # the curve: points read by the count and the emit pass
                T.put(f"roc_k{k}{'_curve' if curve else ''}", T.timed(torch, lambda: eng.roc_k(sc, lb, k=k, curve=curve), reps),
                      sort_bytes(n, passes) + point_bytes + extra)
        T.put("top1", T.timed(torch, lambda: eng.top1(scores, true), reps), n * 4 + NT * 8)
        T.put("top1_labels", T.timed(torch, lambda: eng.top1(scores, true, want_labels=True), reps), n * 5 + NT * 8)
    else:
        res["missing"] = ["svk_roc_k", "svk_top1"]
    T.put("torch_sort", T.timed(torch, lambda: torch.sort(sc, descending=True), reps))

    # end to end on in-memory embeddings: cosine scores -> top-1 -> labels -> ROC (host: sklearn on float64 copies)
    if hasattr(lib, "svk_roc_k") and not os.environ.get("SVK_ROC_SKIP_E2E"):
        speaker_ids = [f"id{j:05d}" for j in range(NS)]
        test_ids = [speaker_ids[j] for j in true.cpu().numpy()]

        def end_to_end(device):
            s = eng.cosine_scores(test, enroll)
            if device:
                return evaluation._device_top1_roc(s, test_ids, speaker_ids, 1, None, False)[:2]
            s = s.cpu().numpy().astype(np.float64)
            lab = evaluation.labels_from_ids(test_ids, speaker_ids)
            correct = int(sum(speaker_ids[int(np.argmax(s[i]))] == test_ids[i] for i in range(NT)))
            return evaluation.get_and_plot_k_eer_auc(lab.flatten(), s.flatten(), k=1, plot_path=None), correct
        import contextlib
        import io
        import time
        with contextlib.redirect_stdout(io.StringIO()):
            T.put("evaluate_device", T.timed(torch, lambda: end_to_end(True), 3, warmup=1))
            t0 = time.perf_counter()
            end_to_end(False)
            res["ms"]["evaluate_host"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["hbm_peak_tb_s"] = T.HBM_PEAK / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()
