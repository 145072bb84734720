"""Score normalisation on a cohort: Z-norm, T-norm and S-norm, adaptive with top_k (the reference has none: its scores are raw
cosines).  The step between the raw score and the calibration: a trial's score is shifted and scaled by the moments of its
two sides' scores against a cohort of impostors, so that one threshold -- one calibration -- serves every speaker.

    side     scores whose moments are taken                          used by
    test     the test row against the cohort                         T-norm, S-norm   (the row table of svk_score_norm)
    enroll   the cohort, as TEST rows, against the enrolled model    Z-norm, S-norm   (the column table)

`svk_cohort_moments` takes the mean and standard deviation of the top_k largest scores of each row (top_k = 0: of all of them,
the non-adaptive forms), `svk_score_norm` / `svk_score_norm_pairs` apply them; the cohort scores come from the scorer the
trials use, `svk_cosine_scores` or `svk_plda_scores`."""


class ScoreNorm:
    MODES = ("z", "t", "s")
    SIDES = ("test", "enroll")
    SCORE_BYTES = 256 << 20            # the rows x cohort score matrix of one chunk stays below this

    def __init__(self, top_k=300, mode="s"):
        """mode: "z" (enrolled side), "t" (test side) or "s" (the mean of the two).  top_k: the cohort scores per row that enter
        the moments, the largest ones; 0 = all of them."""
        if mode not in self.MODES:
            raise ValueError("mode must be one of %s, got %r" % (", ".join(repr(m) for m in self.MODES), mode))
        if int(top_k) != top_k or int(top_k) < 0:
            raise ValueError("top_k must be an integer >= 0 (0: the whole cohort), got %r" % (top_k,))
        self.top_k, self.mode = int(top_k), mode
        self.cohort = self.cohort_counts = self.backend = self.plda = self.eng = None

    def fit(self, cohort_emb, speaker_ids=None, backend=None, plda=None, engine=None):
        """Keeps the cohort as the scorer sees it (`pipeline.project_rows` through `backend` and `plda`, the ones the trials
        are scored with).  cohort_emb: raw embeddings [n, dim].  With speaker_ids [n] the cohort is the speakers' mean models:
        `pipeline.enroll_mean` for the cosine, `Plda.enroll` (with the utterance counts) for PLDA; without, the rows
        themselves.  Returns self."""
        import torch
        from .engine import get_engine
        from .pipeline import enroll_mean, project_rows
        eng = engine or get_engine()
        emb = eng.to_device(cohort_emb, torch.float32)
        if emb.dim() != 2 or emb.shape[0] < 1:
            raise ValueError("the cohort wants [n, dim] embeddings, n >= 1, got %s" % (tuple(emb.shape),))
        counts = None
        if speaker_ids is None:
            cohort = project_rows(eng, emb, backend, plda)
        elif plda is None:
            cohort = project_rows(eng, enroll_mean(emb, speaker_ids)[1], backend, None)
        else:
            _, cohort, counts = plda.enroll(project_rows(eng, emb, backend, None), speaker_ids, engine=eng)
        self.cohort, self.cohort_counts, self.backend, self.plda, self.eng = cohort, counts, backend, plda, eng
        return self

    def _fitted(self):
        if self.cohort is None:
            raise RuntimeError("the score normalisation is not fitted (fit it on a cohort first)")

    def _check_side(self, side):
        if side not in self.SIDES:
            raise ValueError("side must be 'test' or 'enroll', got %r" % (side,))

    def moments(self, rows, side, counts=None):
        """{mean, std} of each row's top_k cohort scores -> float64 [n, 2] on the device.  rows: [n, dim'] as the scorer sees
        them (`VerificationPipeline.project`).  side "test": the rows scored against the cohort.  side "enroll": the rows are
        enrolled models (PLDA: of `counts` utterances each) and the cohort is scored against THEM as test rows -- the Z-norm
        side's definition; the PLDA log-likelihood ratio is not symmetric, so the [cohort, n] scores are formed that way round
        and turned with `.t().contiguous()`, a move of rows that changes no value.  (The cosine is symmetric: no turn.)  The
        scores are formed in row chunks of at most SCORE_BYTES; a row's moments depend on that row alone, so chunking changes
        no bit."""
        import torch
        self._check_side(side)
        self._fitted()
        eng = self.eng
        if self.plda is None and counts is not None:
            raise ValueError("counts belong to PLDA scoring: the cosine does not use them")
        if counts is not None and side != "enroll":
            raise ValueError("counts describe enrolled models: side must be 'enroll'")
        rows = eng.to_device(rows, torch.float32)
        if rows.dim() != 2 or rows.shape[1] != self.cohort.shape[1]:
            raise ValueError("moments wants [n, %d] rows as the scorer sees them, got %s" % (self.cohort.shape[1], tuple(rows.shape)))
        n, n_cohort = int(rows.shape[0]), int(self.cohort.shape[0])
        if counts is not None:
            counts = eng.to_device(counts, torch.int32).reshape(-1)
            if counts.numel() != n:
                raise ValueError("counts holds one entry per enrolled row (%d), got %d" % (n, counts.numel()))
        out = torch.empty((n, 2), dtype=torch.float64, device=eng.device)
        step = max(1, int(self.SCORE_BYTES) // (4 * n_cohort))
        for lo in range(0, n, step):
            part = rows[lo:lo + step]
            if self.plda is None:
                scores = eng.cosine_scores(part, self.cohort)
            elif side == "test":
                scores = self.plda.score(part, self.cohort, counts=self.cohort_counts, engine=eng)
            else:
                scores = self.plda.score(self.cohort, part, counts=None if counts is None else counts[lo:lo + step],
                                         engine=eng).t().contiguous()
            out[lo:lo + step] = eng.cohort_moments(scores, self.top_k)
        return out

    def _tables(self, test_moments, enroll_moments):
        """(row table, column table) of the mode; a side the mode does not use is dropped."""
        row = test_moments if self.mode in ("t", "s") else None
        col = enroll_moments if self.mode in ("z", "s") else None
        if row is None and self.mode != "z":
            raise ValueError("mode %r needs the test moments" % (self.mode,))
        if col is None and self.mode != "t":
            raise ValueError("mode %r needs the enroll moments" % (self.mode,))
        return row, col

    def normalize(self, scores, test_moments, enroll_moments, out=None):
        """scores [n_test, n_enroll] -> the normalised matrix, float32 on the device (svk_score_norm).  out: the tensor to
        write, possibly the scores themselves."""
        self._fitted()
        row, col = self._tables(test_moments, enroll_moments)
        return self.eng.score_norm(scores, row, col, out=out)

    def normalize_trials(self, scores, test_moments, idx_a, enroll_moments, idx_b, out=None, bad_count=None):
        """scores [n_trials] of the trials (test row idx_a[p], enrolled row idx_b[p]) -> normalised, float32 on the device
        (svk_score_norm_pairs): the entry `normalize` gives at (idx_a[p], idx_b[p]), bit for bit."""
        self._fitted()
        row, col = self._tables(test_moments, enroll_moments)
        return self.eng.score_norm_pairs(scores, row, idx_a, col, idx_b, out=out, bad_count=bad_count)

    def side_moments(self, test_rows, enroll_rows, counts=None):
        """The two tables the mode needs from the projected rows of both sides: (test moments or None, enroll moments or None).
        Every row of either side gets its moments, referenced by a trial or not.  The cosine is symmetric: when both sides are
        the SAME tensor (a trial list over one set of embeddings) its one table serves both."""
        test = self.moments(test_rows, "test") if self.mode in ("t", "s") else None
        if test is not None and enroll_rows is test_rows and self.plda is None:
            return test, test
        enroll = self.moments(enroll_rows, "enroll", counts) if self.mode in ("z", "s") else None
        return test, enroll

    def check_scorer(self, backend, plda):
        """Raises unless the normalisation was fitted for the scorer (back end, PLDA) the trials are scored with."""
        self._fitted()
        if self.backend is not backend or self.plda is not plda:
            raise ValueError("the score normalisation was fitted with another back end / PLDA than the scores it is to normalise")
