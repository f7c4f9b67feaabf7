"""The forward half of generate.py as a library call: encode a waveform, quantise it, embed the
condition (optionally for another speaker -- voice conversion, generate.py:19-21, 94-98) and run
the autoregressive decoder on the device.

generate.py's file handling (librosa load/trim, snapshot paths, write_wav) stays outside the hot
path; `serializers.load_npz(path, link, prefix)` loads the reference's snapshot layout
(generate.py:67-81) into the links handed to this function.
"""
import numpy as np

from . import backend, core, ragged
from .core import Variable
from .utils import MuLaw


def _latent_condition(cond, condition_embed):
    """What condition_embed returned, as a generation.LatentCondition, without the full-rate tensor being made (the dense
    tensor it returns for a single latent frame is that frame repeated: its column 0 is taken)."""
    from .generation import LatentCondition
    return LatentCondition.from_condition(cond, condition_embed.local_embed5.W.shape[0], condition_embed.upscale_factor)


def _draw_uniforms(rng, decoder, use_logistic, steps, n):
    """The uniforms of ``steps`` steps of ``n`` sequences as generate.py draws them, (steps, n[, nr_mix]) host doubles; a
    DeviceUniforms is passed through: its numbers are drawn on the device, where they are consumed, and no array
    exists on either side."""
    from .generation import DeviceUniforms
    if isinstance(rng, DeviceUniforms):
        return rng
    if use_logistic:
        return rng.uniform(0, 1, (max(steps, 1), n, decoder.proj2.W.shape[0] // 3))     # generate.py:117
    return rng.random_sample((max(steps, 1), n))                     # inside numpy.random.choice, generate.py:136


def synthesize(encoder, vq, decoder, condition_embed, x_enc, global_condition, rng=None,
               quantize=256, use_logistic=False, n_steps=None, persistent=True, lockstep=False,
               temperature=None, top_k=None, top_p=None, latent_condition=False):
    """generate.py:100-148.

    encoder / vq / decoder / condition_embed: device-resident links (decoder = the WaveNet, EMA or
        target copy as generate.py:70-79 chooses).
    x_enc: host or device float32 (n, 1, T+1, 1) normalised waveform(s) (utils.py:99-100; the
        reference runs n = 1).   global_condition: int32 (n,) speaker ids.
    rng: numpy.random.RandomState (default: a fresh RandomState(), the stand-in for NumPy's global
        RNG that generate.py:117 / 136 draws from).  The uniforms are drawn up front, one per step
        (softmax output) or nr_mix per step (mixture of logistics), in the reference's order.
        A vqvae_amd.DeviceUniforms(seed, stream_ids) is passed through to the decoder instead: nothing is drawn on the
        host, and waveform i's wave depends only on (seed, stream_ids[i]), its own input and the model, not on n or on
        its position.
    lockstep: any number of waveforms; the decoder advances them together through WaveNet.generate_lockstep
        (groups of <= 128) instead of generate_sequence (n <= 4).
    temperature / top_k / top_p: sampling controls, handed to generate_sequence / generate_lockstep as they are (None, a
        scalar or one value per waveform); with any of them generate_sequence leaves the persistent kernel.
    latent_condition: with ``lockstep``, hand the decoder the condition at the latent rate (generation.LatentCondition)
        instead of the full-rate tensor, which is then never made; same waves, bit for bit, 1/80 of the condition's
        memory for the default model.  A ValueError without ``lockstep``: generate_sequence reads the dense tensor.
    Returns (wave, output): wave float64/float32 host array (n, T) as written by generate.py:146-149
        (mu-law expanded for the softmax output), output = the raw sampled bins / values."""
    if latent_condition and not lockstep:
        raise ValueError('synthesize: latent_condition needs lockstep=True (generate_sequence reads the full-rate condition)')
    rng = np.random.RandomState() if rng is None else rng
    xd = x_enc if backend.is_device(x_enc) else backend.to_device(np.asarray(x_enc, np.float32))
    gd = global_condition if backend.is_device(global_condition) else \
        backend.to_device(np.asarray(global_condition, np.int32))
    n = xd.shape[0]
    with core.using_config('train', False), core.no_backprop_mode():
        z = encoder(Variable(xd))                                   # generate.py:95
        e = vq(z)                                                   # generate.py:96
        condition = condition_embed(e, Variable(gd))                # generate.py:97-98
    cond = _latent_condition(condition.data, condition_embed) if latent_condition else condition.data
    T = cond.shape[2]
    steps = T - 1 if n_steps is None else n_steps                   # generate.py:105
    u = _draw_uniforms(rng, decoder, use_logistic, steps, n)
    if lockstep:
        out = decoder.generate_lockstep(cond, u, n_steps=steps, temperature=temperature, top_k=top_k, top_p=top_p)
    else:
        out = decoder.generate_sequence(cond, u, n_steps=steps, persistent=persistent, temperature=temperature,
                                        top_k=top_k, top_p=top_p).get()
    if use_logistic:
        return out, out                                             # generate.py:147
    return MuLaw(quantize).itransform(out), out                     # generate.py:149


def synthesize_many(encoder, vq, decoder, condition_embed, waves, global_condition, rng=None,
                    quantize=256, use_logistic=False, n_steps=None, group=128, refill=True,
                    temperature=None, top_k=None, top_p=None, return_output=False, latent_condition=False,
                    batched_frontend=False):
    """``synthesize`` for a list of waveforms of different lengths (a validation set, a corpus).

    waves: list of N normalised waveforms, each a host or device float32 array of T_i + 1 samples (any shape that
        holds them).  global_condition: int32 (N,) speaker ids.
    Each waveform is encoded, quantised and condition-embedded on its own, with n = 1: in a padded batch the encoder's
    and ConditionEmbed's edge samples and the align-corners up-sampling would see the padding.  The condition rows are
    packed into one zero-padded (N, condition_dim, Tmax) device array and the decoder runs them with their lengths
    through WaveNet.generate_lockstep; ``refill`` (default True) keeps its ``group`` columns busy by handing a finished
    column the next waiting utterance.
    rng: as in synthesize; the uniforms are drawn as it draws them for shape (Tmax - 1, N[, nr_mix]), so utterance i
        uses column i, and its wave depends on how many utterances the list has and on the longest one.
        A vqvae_amd.DeviceUniforms(seed, stream_ids) is passed through to the decoder instead: nothing is drawn on the
        host (for 300 utterances of up to 10 s that array is 384 MB, 3.8 GB with a mixture of 10 logistics, and the same
        again on the device), and utterance i's wave depends only on (seed, stream_ids[i]), its own input and the
        model, not on the list: the same bits alone, in any list, at any position, with any ``group`` and ``refill``.
    latent_condition: keep the condition at the latent rate (generation.LatentCondition): no utterance's condition is
        expanded to the sample rate, the (N, condition_dim, Tmax) array and its N * condition_dim row copies do not
        exist, and the decoder computes each step's condition column on the device.  Same waves, bit for bit.
        Recommended for corpora: the dense array takes 2 560 bytes per sample of the LONGEST utterance times N for the
        default model (123 GB for 300 utterances of up to 10 s at 16 kHz), the latent form 32 bytes per sample of each
        utterance.  On the default decoder the step is also a quarter faster with it (the gate launches read a
        contiguous column).  The default is False because the call without it is the call as it was.
    batched_frontend: with ``latent_condition``, encode, quantise and embed ALL utterances per launch
        (frontend.frontend_many: the ragged convs of include/vqvae_ragged.h, where every tap stays inside its own
        utterance) instead of one utterance at a time with n = 1: 12 calls and two uploads (waves, tables) per chunk instead
        of about 20 launches and two uploads per utterance.  A ValueError without ``latent_condition``.  The default is
        False: the call without it launches exactly what it launched before.
    Returns the list of N host waves, utterance i of its own length T_i, as synthesize returns them (mu-law expanded
    for the softmax output); with ``return_output`` the list of (wave, output) pairs."""
    rng = np.random.RandomState() if rng is None else rng
    N = len(waves)
    speakers = np.asarray(global_condition.get() if backend.is_device(global_condition) else global_condition,
                          np.int32).reshape(-1)
    if speakers.shape != (N,):
        raise ValueError('synthesize_many: one speaker id per waveform (%d), got %s' % (N, speakers.shape))
    if batched_frontend and not latent_condition:
        raise ValueError('synthesize_many: batched_frontend needs latent_condition=True (the ragged front end writes the '
                         'latent-rate condition)')
    conds = []
    with core.using_config('train', False), core.no_backprop_mode():
        for w, spk in ([] if batched_frontend else zip(waves, speakers)):
            xd = w if backend.is_device(w) else backend.to_device(np.asarray(w, np.float32))
            xd = xd.reshape(1, 1, xd.size, 1)
            e = vq(encoder(Variable(xd)))                                                  # generate.py:95-96
            c = condition_embed(e, Variable(backend.to_device(np.array([spk], np.int32)))).data   # generate.py:97-98
            conds.append(_latent_condition(c, condition_embed) if latent_condition else c.reshape(c.shape[1], c.shape[2]))
    if batched_frontend:
        from .frontend import frontend_many
        cond = frontend_many(encoder, vq, condition_embed, waves, speakers)
        lengths = cond.lengths
        Tmax = cond.shape[2]
    elif latent_condition:
        from .generation import LatentCondition
        cond = LatentCondition.concatenate(conds)
        lengths = cond.lengths
        Tmax = cond.shape[2]
    else:
        lengths = np.array([c.shape[1] for c in conds], np.int64)
        Tmax = int(lengths.max())
        cond = ragged.pack_padded(conds, lengths, conds[0].shape[0], Tmax)
    steps = Tmax - 1 if n_steps is None else n_steps
    u = _draw_uniforms(rng, decoder, use_logistic, steps, N)
    out = decoder.generate_lockstep(cond, u, n_steps=n_steps, lengths=lengths, group=group, refill=refill,
                                    temperature=temperature, top_k=top_k, top_p=top_p)
    wave = out if use_logistic else MuLaw(quantize).itransform(out)
    res = [(wave[i, :L], out[i, :L]) for i, L in enumerate(lengths)]
    return res if return_output else [w for w, _ in res]
