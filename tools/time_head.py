"""HIP-event medians of C3D2's classification head at dev-set scale (148 642 seeded embeddings, 128 dims) for 1 211 and 100
labels: svk_c3d2_head with the probabilities written or not, k = 1 and 5, against the torch head it replaces (F.linear +
softmax + argmax / topk on the same tensors).  Next to each time: the FLOP of the FC6 GEMM as the kernel issues it (three
passes over the logits: DESIGN 3.7) and as torch issues it (one), the bytes each moves by its design, TF/s and TB/s.

SVK_TOOL_LIB=path/to/libsvk.so times another build (e.g. under build_variants/); a build without svk_c3d2_head reports it
missing.  One JSON line on stdout."""
import json
import os

import _timing as T          # (puts the repository on sys.path)

N, D = 148642, 128


def main():
    import torch
    import torch.nn.functional as F
    _lib, lib = T.load_lib()
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    reps = int(os.environ.get("SVK_HEAD_REPS", "10"))
    g = torch.Generator(device=eng.device).manual_seed(3)
    emb = torch.randn(N, D, device=eng.device, generator=g)
    res = T.header(_lib, lib, sha=False, n=N, ms={}, tf_s={}, tb_s={})
    have = hasattr(lib, "svk_c3d2_head")
    if not have:
        res["missing"] = ["svk_c3d2_head"]

    for n_labels in (1211, 100):
        w = 0.1 * torch.randn(n_labels, D, device=eng.device, generator=g)
        b = 0.5 * torch.randn(n_labels, device=eng.device, generator=g)
        slope = torch.tensor([0.25], device=eng.device)
        tables = (w, b, 0.25)
        gemm = 2.0 * N * n_labels * D
        base = N * D * 4 + n_labels * (D + 1) * 4                  # embeddings + the tables, read once
        probs_bytes = N * n_labels * 4
        if have:
            for probs in (True, False):
                for k in (1, 5):
                    name = "head_%d_%s_k%d" % (n_labels, "probs" if probs else "noprobs", k)
                    T.put(name, T.timed(torch, lambda: eng.c3d2_head(emb, tables, probs=probs, k=k), reps),
                            base + (probs_bytes if probs else 0) + N * k * 4, 3 * gemm)

        def torch_head(k):
            p = F.softmax(F.linear(F.prelu(emb, slope), w, b), dim=1)
            return p, (torch.argmax(p, 1) if k == 1 else torch.topk(p, k, 1)[1])
        # logits written and read by softmax, probabilities written and read by the argmax / topk
        for k in (1, 5):
            T.put("torch_%d_k%d" % (n_labels, k), T.timed(torch, lambda: torch_head(k), reps),
                    base + 4 * probs_bytes + N * k * 8, gemm)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
