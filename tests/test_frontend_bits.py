"""The bits of the fused front end (csrc/frontend.hip, svk_frontend_run), pinned for refactors: the SHA-256 of the bytes of
`feat`, `n_frames` and, where it is asked for, `energy` of every launch against tests/golden/frontend_bits.json.

The golden pins ONE compiler and ONE architecture (hipcc of the ROCm release the digests were recorded with, gfx950): a change
that leaves the source's arithmetic and its order alone leaves these digests alone, and a deliberate change of the arithmetic
order or a compiler that contracts or reorders differently must re-record the file -- run this module once on the commit BEFORE
such a change with SVK_FRONTEND_BITS_RECORD=1 to see that it reproduces the committed file, and once after it to write the new
one.  What the numbers should be is the business of tests/test_frontend_float64.py; this file only says they are still the same.

The launches are exactly those of test_frontend_float64.py's GPU tests, on that module's inputs (its case tables, ragged_batch,
ticket_batch, set_env, padded and launch are imported, not restated):
  * SPECIALISED x {plain, pre-emphasis}: the specialised instance, the generic one forced for the same input, and the log-mel
    configuration falling back to the generic instance when the frame energies are asked for;
  * every GENERIC_CASES entry (tile 8 / 16 with an Engine per tile, the four stagings, the output kinds, dc_elimination, the
    energy request) and every GEOMETRIES entry;
  * the two max_frames cases on a specialised and a generic instance;
  * the gathered-input case: plain, identity table, the selection copied out, the selection through the table;
  * the ticket batch with one wave per workgroup and with the library's wave count.
Every digest is recorded together with the instance that the library's debug line names, and the instance is asserted before
the digest is compared: a digest cannot silently come from another instance."""
import hashlib
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_frontend_float64 as F                                # noqa: E402  (tests/ is on sys.path)
from test_frontend_float64 import engines                        # noqa: E402,F401  (the module-scoped Engine-per-tile fixture)
from speaker_verification_amd import synth                       # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_bits.json")
RECORD = bool(os.environ.get("SVK_FRONTEND_BITS_RECORD"))

CHUNK, N_CHUNKS = 160, 50
_GATHERED = []


def gathered_inputs():
    """test_gathered_input_is_bit_identical's inputs: four clips of 2 x 50 chunks, the gathered lengths (one of them 0), and
    the table that picks every other chunk (the odd ones for odd clips)."""
    if not _GATHERED:
        n = 2 * CHUNK * N_CHUNKS
        long = np.stack([synth.noise_clip(500, n), synth.speaker_clip(3, 1, n), F._tone_noise(9, n), synth.noise_clip(501, n)])
        lens = np.array([CHUNK * N_CHUNKS, CHUNK * 31 + 77, 0, CHUNK * 7 + 159], dtype=np.int32)
        table = np.stack([2 * np.arange(N_CHUNKS) + (u & 1) for u in range(len(long))]).astype(np.int32)
        picked = np.stack([long[u].reshape(-1, CHUNK)[table[u]].reshape(-1) for u in range(len(long))])
        _GATHERED.append((long, lens, table, picked))
    return _GATHERED[0]


def launches():
    """Every launch as a dict: name, expect (the instance), spec, energy, and what differs from the defaults -- batch (a
    ragged_batch name) or clips (a callable), env (set_env's keywords), tile (the Engine), M (max_frames), gather."""
    out = []

    def add(name, expect, spec, energy, **kw):
        out.append(dict(name=name, expect=expect, spec=spec, energy=energy, **kw))

    for name, mk, f32 in F.SPECIALISED:
        for pre in (False, True):
            spec = mk(**(F.PRE if pre else {}))
            batch = F.batch_for(spec, f32)
            energy = spec.out_kind == F.MFCC
            tag = "specialised-%s-%s" % (name.replace(" ", ""), "preemph" if pre else "plain")
            add(tag, name, spec, energy, batch=batch)
            add(tag + "-forced_generic", "generic", spec, energy, batch=batch, env=dict(generic=1))
            if spec.out_kind == F.LMFE:
                add(tag + "-energy_asked", "generic", spec, True, batch=batch)
    for c in F.GENERIC_CASES:
        cfg, tile, st, spec, energy = c
        add("generic-" + F._id(c), "generic", spec, energy, batch=F.batch_for(spec, st == "f32"), tile=tile,
            env=dict(generic=1, tile=tile, f32stage=1 if st == "i16 f32stage" else None))
    for what, spec in F.GEOMETRIES:
        add("geometry-" + what.replace(" ", "_"), "generic", spec, True, batch=F.batch_for(spec), env=dict(generic=1))
    for M in (40, 120):
        add("max_frames-%d-mfcc13" % M, "mfcc13", F.spec_a(**F.PRE), True, batch="i320", M=M)
        add("max_frames-%d-generic-B" % M, "generic", F.spec_b(F.MFCC, **F.PRE), True, batch="f400", M=M)
    gathered = (("preemph-A", "mfcc13", F.spec_a(**F.PRE)), ("preemph-B", "generic", F.spec_b(**F.PRE)),
                ("mfe-A", "generic", F.spec_a(F.MFE)), ("mfcc-B", "generic", F.spec_b(F.MFCC)))
    for tag, expect, spec in gathered:      # (spec_b with the energy asked for leaves the log-mel instance)
        for how in ("plain", "identity", "picked", "every_other"):
            add("gathered-%s-%s" % (tag, how), expect, spec, True, gather=how, M=spec.num_frames(CHUNK * N_CHUNKS))
    for waves in (1, None):
        for spec in F.ticket_specs():
            add("ticket-%s-%s" % ("one_wave" if waves == 1 else "library_waves", F._id(("-", 8, "", spec, True))),
                "mfcc13" if spec.out_kind == F.MFCC else "lmfe40", spec, spec.out_kind == F.MFCC, batch="ticket",
                env=dict(waves=waves))
    return out


LAUNCHES = launches()
assert len(set(c["name"] for c in LAUNCHES)) == len(LAUNCHES)


def run(eng, capfd, c):
    """-> (instance, digest) of one launch."""
    kw = dict(want_energy=c["energy"], max_frames=c.get("M"))
    how = c.get("gather")
    if how is None:
        clips = F.ragged_batch(c["batch"])[0]
    else:
        long, lens, table, picked = gathered_inputs()
        clips = list({"plain": long[:, :CHUNK * N_CHUNKS], "identity": long[:, :CHUNK * N_CHUNKS], "picked": picked,
                      "every_other": long}[how])
        kw["lengths"] = lens
        if how == "identity":
            ident = torch.arange(N_CHUNKS, dtype=torch.int32, device=eng.device).repeat(len(clips), 1).contiguous()
            kw["gather"] = (ident, CHUNK)
        elif how == "every_other":
            kw["gather"] = (eng.to_device(table), CHUNK)
    feat, nf, en, inst, _, _ = F.launch(eng, capfd, clips, c["spec"], **kw)
    assert (en is not None) == c["energy"]
    h = hashlib.sha256()
    for a in (feat, nf) + ((en,) if c["energy"] else ()):
        h.update(np.ascontiguousarray(a).tobytes())
    return inst, h.hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(LAUNCHES)), ids=[c["name"] for c in LAUNCHES])
def test_output_bits_are_the_recorded_ones(engines, monkeypatch, capfd, index):
    """The launch ran on the instance it names, and its output bytes hash to the recorded digest."""
    c = LAUNCHES[index]
    F.set_env(monkeypatch, **c.get("env", {}))
    inst, got = run(engines(c.get("tile")), capfd, c)
    assert inst == c["expect"], (c["name"], inst)
    if RECORD:
        gold = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
        gold.setdefault("digests", {})[c["name"]] = {"instance": inst, "sha256": got}
        gold["hip_runtime"] = torch.version.hip
        gold["arch"] = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
        with open(GOLDEN, "w") as f:
            json.dump(gold, f, indent=1, sort_keys=True)
            f.write("\n")
    gold = json.load(open(GOLDEN))["digests"]
    assert RECORD or set(gold) == set(x["name"] for x in LAUNCHES)
    assert gold[c["name"]]["instance"] == inst, "%s: recorded on the %s instance" % (c["name"], gold[c["name"]]["instance"])
    assert got == gold[c["name"]]["sha256"], "%s: other bits than recorded" % c["name"]
