"""Float64 references and scalar restatements for whole-recording feature extraction (cpc_audio_amd.feature_extraction; DESIGN.md,
"Whole-recording feature extraction"), shared by test_feature_extraction_host.py and test_feature_extraction_gpu.py.

  scalar_schedule     the host schedule once more, as a step-by-step simulation of the streams and their queue (no numpy arithmetic)
  check_table         the schedule's properties, asserted on a table
  whole_reference     oracle.cpc_oracle.encoder_forward on a whole recording, then the context network stepped over all its frames
                      (gru_stacked_reference.stacked_gru_forward / lstm_reference.lstm_model_reference, one frame per call with the
                      states handed on, which is what gives the state after EVERY frame)
  chunked_reference   the same computed the way the extractor does: windows of samples per chunk, states handed from chunk to chunk
                      (hand_off=False: every chunk from zero states, the bug the hand-off tests look for)
References are computed once per key and never modified.
"""
import numpy as np
import torch

from oracle import cpc_oracle as O
import gru_stacked_reference as GS
import lstm_reference as LR

E_S = 64
SMALL = {'strides': [5, 4, 2, 2, 2], 'kernel_sizes': [10, 8, 4, 4, 4], 'channel_count': [E_S] * 5, 'bias': True}          # test_lstm_gpu.py's
DS, RF = O.encoder_geometry(SMALL['strides'], SMALL['kernel_sizes'])
LSTM_PREFIX = "autoregressive_model.lstmCell."


def frames_of(n, rf=RF, ds=DS):
    return (n - rf) // ds + 1 if n >= rf else 0


def samples_for(frames, rf=RF, ds=DS, extra=0):
    """A length that gives exactly ``frames`` frames (0: one sample short of a receptive field); extra < ds more samples change nothing."""
    return rf - 1 if frames == 0 else (frames - 1) * ds + rf + extra


# ----------------------------------------------------------------------------------------------------------------------- schedule
def scalar_schedule(first_samples, lengths, rf, ds, R, Tc):
    """[n_steps][R][6] as nested lists: at every step each stream, lowest first, that has no recording takes the next one with frames
    from the queue; a stream with a recording does its next chunk."""
    frames = [frames_of(n, rf, ds) for n in lengths]
    offsets = [0]
    for f in frames:
        offsets.append(offsets[-1] + f)
    queue = [i for i, f in enumerate(frames) if f > 0]
    current = [None] * R          # per stream: (recording, frames done)
    steps = []
    while queue or any(c is not None for c in current):
        rows = []
        for r in range(R):
            if current[r] is None and queue:
                current[r] = (queue.pop(0), 0)
            if current[r] is None:
                rows.append([0, 0, 0, 0, -1, 0])
                continue
            i, done = current[r]
            nf = min(Tc, frames[i] - done)
            more = done + nf < frames[i]
            rows.append([first_samples[i] + done * ds, (nf - 1) * ds + rf, nf, offsets[i] + done, i, 1 if more else 0])
            current[r] = (i, done + nf) if more else None
        steps.append(rows)
    return steps, frames, offsets


def check_table(table, first_samples, lengths, rf, ds, R, Tc):
    """Every frame of every recording exactly once, in order, on one stream, on consecutive steps; windows inside their files; keep
    exactly where the stream's next row continues the recording; output rows a partition of [0, total_frames)."""
    table = np.asarray(table).reshape(-1, R, 6)
    frames = [frames_of(n, rf, ds) for n in lengths]
    total = sum(frames)
    covered = np.zeros(total, dtype=np.int64)
    seen = {}          # recording -> (stream, last step, frames done)
    for j in range(table.shape[0]):
        recs = [int(v) for v in table[j, :, 4] if v >= 0]
        assert len(recs) == len(set(recs)), "a recording on two streams in one step"
        for r in range(R):
            first, n, nf, out, rec, keep = (int(v) for v in table[j, r])
            if rec < 0:
                assert (first, n, nf, out, keep) == (0, 0, 0, 0, 0)
                continue
            assert 0 <= rec < len(lengths) and 1 <= nf <= Tc
            stream, last, done = seen.get(rec, (r, j - 1, 0))
            assert stream == r and last == j - 1, "a recording left its stream or skipped a step"
            assert first == first_samples[rec] + done * ds and n == (nf - 1) * ds + rf
            assert first_samples[rec] <= first and first + n <= first_samples[rec] + lengths[rec], "window outside its file"
            assert out == sum(frames[:rec]) + done
            covered[out:out + nf] += 1
            done += nf
            assert keep == (1 if done < frames[rec] else 0)
            if keep:
                assert j + 1 < table.shape[0] and int(table[j + 1, r, 4]) == rec
            else:
                assert nf == Tc or done == frames[rec]
                assert j + 1 == table.shape[0] or int(table[j + 1, r, 4]) != rec
            if done < frames[rec]:
                assert nf == Tc, "a short chunk that is not the recording's last"
            seen[rec] = (r, j, done)
    assert (covered == 1).all(), "output rows are not a partition of [0, total_frames)"
    assert all(seen[i][2] == f for i, f in enumerate(frames) if f > 0) and all(i not in seen for i, f in enumerate(frames) if f == 0)


# ---------------------------------------------------------------------------------------------------------------------- reference
def _double(params):
    return {k: v.detach().double().cpu() for k, v in params.items()}


def _zero_state(kind, layers, H):
    z = lambda: torch.zeros(1, H, dtype=torch.float64)
    return (z(), z()) if kind == "lstm" else [z() for _ in range(layers)]


def _context_steps(z, params, kind, layers, state):
    """z (1, E, F) float64 -> (c (F, H): the top state after every frame, the states after the last frame)."""
    out = []
    for t in range(z.shape[2]):
        frame = z[:, :, t:t + 1]
        if kind == "lstm":
            state = LR.lstm_model_reference(frame, params, prefix=LSTM_PREFIX, h0=state[0], c0=state[1])
            out.append(state[0][0])
        else:
            _, state = GS.stacked_gru_forward(frame, params, layers, h0=state, return_states=True)
            out.append(state[-1][0])
    H = (state[0] if kind == "lstm" else state[-1]).shape[1]
    return (torch.stack(out) if out else torch.zeros(0, H, dtype=torch.float64)), state


def _encode(samples, params, cfg):
    x = torch.as_tensor(samples, dtype=torch.float64).view(1, 1, -1)
    return O.encoder_forward(x, params, strides=cfg['strides'])


def whole_reference(samples, params, kind, layers=1, cfg=SMALL):
    """(z (F, E), c (F, H)) of one recording in float64: the encoder on the whole recording, the context over all frames from zero
    states.  ``samples``: float values (int16 already scaled)."""
    params = _double(params)
    rf, ds = O.encoder_geometry(cfg['strides'], cfg['kernel_sizes'])[::-1]
    H = params[(LSTM_PREFIX if kind == "lstm" else "autoregressive_model.gruCell.") + "weight_hh"].shape[1]
    if len(samples) < rf:
        return torch.zeros(0, cfg['channel_count'][-1], dtype=torch.float64), torch.zeros(0, H, dtype=torch.float64)
    with torch.no_grad():
        z = _encode(samples, params, cfg)
        c, _ = _context_steps(z, params, kind, layers, _zero_state(kind, layers, H))
    return z[0].T.contiguous(), c


def chunked_reference(samples, params, kind, Tc, layers=1, cfg=SMALL, hand_off=True):
    """The same, chunk by chunk as the extractor schedules it: chunk k covers frames [k Tc, min((k + 1) Tc, F)) and is computed from
    samples [k Tc ds, + (n_frames - 1) ds + rf) alone; the states go from chunk to chunk (hand_off=False: every chunk starts at zero)."""
    params = _double(params)
    ds, rf = O.encoder_geometry(cfg['strides'], cfg['kernel_sizes'])
    H = params[(LSTM_PREFIX if kind == "lstm" else "autoregressive_model.gruCell.") + "weight_hh"].shape[1]
    F = frames_of(len(samples), rf, ds)
    zs, cs = [torch.zeros(0, cfg['channel_count'][-1], dtype=torch.float64)], [torch.zeros(0, H, dtype=torch.float64)]
    state = _zero_state(kind, layers, H)
    with torch.no_grad():
        for f0 in range(0, F, Tc):
            nf = min(Tc, F - f0)
            z = _encode(samples[f0 * ds:f0 * ds + (nf - 1) * ds + rf], params, cfg)
            assert z.shape[2] == nf
            c, state = _context_steps(z, params, kind, layers, state if hand_off else _zero_state(kind, layers, H))
            zs.append(z[0].T)
            cs.append(c)
    return torch.cat(zs), torch.cat(cs)


def pooled_reference(x):
    """(mean, population deviation) per channel of (F, C) float64 rows; zeros for F = 0."""
    if x.shape[0] == 0:
        return torch.zeros(x.shape[1], dtype=torch.float64), torch.zeros(x.shape[1], dtype=torch.float64)
    mean = x.mean(0)
    return mean, ((x * x).mean(0) - mean * mean).clamp(min=0).sqrt()


def rel_l2(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-30)).item()


# --------------------------------------------------------------------------------------------------------------------------- data
FRAME_COUNTS = (0, 1, 5, 16, 37, 64)          # the end-to-end recordings


def recordings(frame_counts=FRAME_COUNTS, seed=7):
    """int16 recordings with the given frame counts (each with a few samples more than its frames need, so that the frame-count
    arithmetic's floor is exercised), amplitude about 0.5 of full scale / 3."""
    g = np.random.default_rng(seed)
    return [np.clip(g.standard_normal(samples_for(f, extra=(3 * k) % DS if f else 0)) * 5000.0, -32768, 32767).astype(np.int16)
            for k, f in enumerate(frame_counts)]


def model_for(kind, H=32, layers=1, dtype="fp32", seed=3):
    """The small encoder of test_lstm_gpu.py (64 channels, encoder weights doubled) with a GRU (``layers``) or LSTM context of size H,
    context weights scaled up so that the state depends visibly on its past (see test_hand_off_matters_in_the_reference)."""
    from cpc_audio_amd.audio_model import AudioEncoder, AudioGRUModel, AudioLSTMModel, AudioPredictiveCodingModel
    torch.manual_seed(seed)
    ar = AudioLSTMModel(E_S, H) if kind == "lstm" else AudioGRUModel(E_S, H, num_layers=layers)
    model = AudioPredictiveCodingModel(AudioEncoder(SMALL), ar, enc_size=E_S, ar_size=H, visible_steps=12, prediction_steps=4,
                                       compute_dtype=dtype)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.startswith("encoder.") and n.endswith("weight"):
                p.mul_(2.0)
            if n.startswith("autoregressive_model.") and n.endswith("weight_hh"):
                p.mul_(CONTEXT_SCALE)
    return model


CONTEXT_SCALE = 2.0          # recurrent weights times this: the state's memory reaches across a chunk boundary


_REFS = {}


def reference_features(kind, layers, params, recs):
    """[(z, c)] per recording, float64, computed once per (kind, layers)."""
    key = (kind, layers)
    if key not in _REFS:
        _REFS[key] = [whole_reference(r.astype(np.float64) / 32768.0, params, kind, layers) for r in recs]
    return _REFS[key]
