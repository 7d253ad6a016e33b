"""Batch command-line tools over the reference's file formats.

The reference ships one-file-at-a-time programs (examples/parameter_io/f0analysis.cpp,
spanalysis.cpp, apanalysis.cpp, readandsynthesis.cpp); these do the same work for MANY files
per call, batched on the GPU, and read / write the same F0 / SPEC / AP / WAV files:

    python -m world_amd.tools analysis a.wav b.wav ... --outdir params      # -> params/a.f0 a.sp a.ap ...
    python -m world_amd.tools synthesis params/a.f0 params/a.sp params/a.ap -o a_resynth.wav
    python -m world_amd.tools transform a.wav b.wav ... --outdir out --f0-scale 1.5 --formant-shift 1.2
    python -m world_amd.tools transform a.wav --outdir out --duration 2.5 --f0-from melody.f0
    python -m world_amd.tools transform a.wav --outdir out --align-to b.wav       # a's voice with b's timing
    python -m world_amd.tools mcd ref1.wav test1.wav ref2.wav test2.wav --dims 25 # mel-cepstral distortion along the DTW path
    python -m world_amd.tools morph a.wav b.wav -o out.wav --rate 0.3             # 70 % a, 30 % b; --fade: a cross-fades into b
    python -m world_amd.tools resample a.wav b.wav ... --outdir out --fs 16000    # every file at 16 kHz (--quality fast|best)
    python -m world_amd.tools morph a44k.wav b48k.wav -o out.wav --fs 48000       # --fs on analysis, transform, mcd, morph
    python -m world_amd.tools features a.wav b.wav ... --outdir feats --order 59  # -> feats/a.lf0 a.mgc a.bap (float32)
    python -m world_amd.tools features-synthesis a.lf0 a.mgc a.bap --fs 48000 --order 59 -o a.wav
    python -m world_amd.tools mcd ref.wav test.wav --mcep 24                      # MCD on all-pass mel-cepstra c1 .. c24
    python -m world_amd.tools deltas a.mgc --dim 60 -o a.mgc.dyn                  # [frames][60] -> [frames][180]: static, delta, delta-delta
    python -m world_amd.tools mlpg mean.mgc.dyn var.mgc.dyn --dim 60 -o a.mgc     # the smooth trajectory under means and variances
    python -m world_amd.tools vc-train s1.mgc s2.mgc --target t1.mgc t2.mgc --dim 25 --mix 32 --iter 20 -o model.npz
    python -m world_amd.tools vc-train s*.mgc --target t*.mgc --dim 25 --power-gate -20 --fs 16000 --realign 2 -o model.npz
    python -m world_amd.tools vc-convert model.npz s3.mgc --dim 25 -o s3_as_t.mgc   # goes into features-synthesis as it is

`analysis` keeps the example programs' option letters where they exist (-f/-c/-s of f0analysis,
-q of spanalysis, -t of apanalysis).  Files are grouped by sampling rate; only their PCM bytes
are uploaded (decoded on the device), and with --code-sp / --code-ap the envelopes are coded on
the device before they come back, so the D2H traffic and the files shrink by 10-17x.
`transform` is the reference test program's analysis -> ParameterModification -> Synthesis (F0 scale, formant shift,
and a speed change through the synthesis frame period) in one library call per batch; the waveforms are quantised to
16 bits on the device, so only int16 samples come back.  With --duration or --f0-from the modification is per frame
(world_hip_resynthesize_frames_batch): a uniform time map to the asked length, and the F0 track of another file as target.
With --align-to the time map is the alignment of each input to another recording (world_hip_align_batch over the
mel-cepstra of both, c0 left out), one output frame per frame of that recording.  `mcd` analyses pairs of files into coded
records, aligns each pair on the device and prints the mel-cepstral distortion along the path.  `morph` analyses two files, aligns them the same way and writes the frames
between them (world_hip_morph_batch): timing, F0, envelope and aperiodicity each part-way from the first file to the second.
`resample` converts files to one sampling rate (world_hip_resample_batch, a polyphase Kaiser-windowed sinc): PCM bytes go
up, decode, conversion and the 16-bit quantiser run on the device, int16 comes down.  `analysis`, `transform`, `mcd` and
`morph` take --fs F (and --quality): every input whose rate differs from F is converted on the device between the PCM decode
and the analysis -- nothing is quantised in between -- so files of any rates can be used together (and an 8 kHz recording,
below D4C's range, analysed at 16 kHz).  Files are still batched per SOURCE rate, one conversion per batch; outputs carry F.
Without --fs every tool behaves as before, refusals of mixed rates included.
`features` writes what TTS and voice-conversion corpora are stored in, headerless little-endian float32 (the HTS / Merlin
convention): .lf0 = ln F0 per frame, -1e10 where unvoiced; .mgc = [frames][order + 1] mel-cepstra by all-pass warping
(world_hip_sp2mc: SPTK's freqt, what other WORLD bindings call sp2mc; alpha defaults to world_hip_mcep_alpha of the rate);
.bap = CodeAperiodicity's band values.  `features-synthesis` is the way back (world_hip_mc2sp, DecodeAperiodicity, synthesis).
`mcd --mcep M` scores c1 .. cM of those cepstra instead of the reference coder's, the figure published MCDs are computed on;
the alignment itself is unchanged.
`deltas` appends the dynamic features acoustic models are trained on (world_hip_delta_batch, windows [1], [-0.5 0 0.5],
[1 -2 1]) to a float32 file of [frames][dim] statics; `mlpg` is the way back from a model's output (world_hip_mlpg_batch,
maximum-likelihood parameter generation): a file of [frames][3 dim] means and one of as many rows, or of one row, of
variances give the [frames][dim] trajectory, which goes into `features-synthesis` as it is.  With --lf0 (dim 1) the -1e10
frames are masked: windows stop at the ends of every voiced run and unvoiced frames stay -1e10.
`vc-train` fits the classic joint-density Gaussian mixture of voice conversion (world_hip_gmm_fit) on pairs of .mgc files of
two speakers: the deltas of every utterance, ONE world_hip_align_batch call over the statics without c0 of all pairs, one
world_hip_joint_rows_batch call for the joint rows [x, dx, y, dy] along the paths; all rows of all pairs are fitted together and
w, mu, cov and the dimensions saved as .npz.  With --power-gate DB --fs F each speaker's frames below DB dB of their utterance's
mean power (world_hip_frame_power_batch on the envelope of the cepstra, world_hip_select_frames_batch) stay out of the alignment
and the rows (-20: the usual silence gate; the deltas are still those of the whole utterance).  With --realign R the sources
are converted with the fitted model, the converted frames aligned to the targets, the rows rebuilt from the original source
features along the new paths and the model refitted from where it stood, R times; each round prints its mean log-likelihood
and the mean MCD along the paths.  Without either option the model is the one earlier versions saved.  `vc-convert` turns a
source .mgc into the target speaker's: deltas, world_hip_gmm_convert (the per-frame means and variances of [y, dy]), mlpg.
There is no CPU path: without a GPU and the built library this exits with an error.
"""
import argparse
import os
import sys

import numpy as np

from .api import FileAPI, WorldHip, cheaptrick_fft_size, frame_count, uniform_time_map


def _at_rate(wh, x, x_len, fs, target, quality="best"):
    """--fs: a decoded batch of rate fs -> (x, x_len, rate) at the target rate (None or the batch's own: as it is)"""
    if target is None or target == fs:
        return x, x_len, fs
    try:
        y, y_len = wh.resample(x, fs, target, x_len=x_len, quality=quality)
    except RuntimeError as e:                                   # the library's refusal (44100 -> 48001 Hz: too many phases)
        raise ValueError(str(e)) from None
    return y, y_len, target


def _check_rate(tool, a):
    if a.fs is not None and a.fs < 1:
        sys.exit(f"{tool}: --fs {a.fs} is not a sampling rate")


def _analysis(a):
    _check_rate("analysis", a)
    wh, files = WorldHip(), FileAPI()
    os.makedirs(a.outdir, exist_ok=True)
    by_rate = {}
    for path in a.wav:
        by_rate.setdefault(wh.wav_layout(path)[0], []).append(path)
    frames = 0
    for src_fs, group in sorted(by_rate.items()):
        for at in range(0, len(group), a.batch):
            chunk = group[at:at + a.batch]
            x, x_len = _load_batch(wh, chunk)
            try:
                x, x_len, fs = _at_rate(wh, x, x_len, src_fs, a.fs, a.quality)
            except ValueError as e:
                sys.exit(f"analysis: {e}")
            tpos, f0, sp, ap, nf = wh.analyze(x, fs, x_len=x_len, f0_method=a.f0, frame_period=a.s, f0_floor=a.f,
                                              f0_ceil=a.c, q1=a.q, threshold=a.t)
            fft_size = cheaptrick_fft_size(fs, 71.0)
            sp_dims = ap_dims = 0
            if a.code_sp:
                sp, sp_dims = wh.code_spectral_envelope(sp, fs, fft_size, a.code_sp), a.code_sp
            if a.code_ap:
                ap = wh.code_aperiodicity(ap, fs, fft_size)
                ap_dims = ap.shape[-1]
            tpos, f0, sp, ap = (t.cpu().numpy() for t in (tpos, f0, sp, ap))
            for row, path in enumerate(chunk):
                n, stem = int(nf[row]), os.path.join(a.outdir, os.path.splitext(os.path.basename(path))[0])
                files.write_f0(stem + ".f0", a.s, tpos[row, :n], f0[row, :n], text=a.text)
                files.write_spectral_envelope(stem + ".sp", sp[row, :n], fs, a.s, fft_size, sp_dims)
                files.write_aperiodicity(stem + ".ap", ap[row, :n], fs, a.s, fft_size, ap_dims)
                frames += n
    print(f"{len(a.wav)} file(s), {frames} frames -> {a.outdir}")


def _synthesis(a):
    import torch
    wh, files = WorldHip(), FileAPI()
    fs, fft_size = int(files.header(a.sp, "FS  ")), int(files.header(a.sp, "FFT "))
    frame_period = files.header(a.sp, "FP  ")
    read = files.read_f0(a.f0)
    sp, ap = files.read_spectral_envelope(a.sp), files.read_aperiodicity(a.ap)
    if read is None or sp is None or ap is None:
        sys.exit("synthesis: unreadable parameter file")
    n = len(read[1])
    y_length = int(n * frame_period / 1000.0 * fs)              # examples/parameter_io/readandsynthesis.cpp:85
    if int(files.header(a.sp, "NOD ")) and int(files.header(a.ap, "NOD ")):
        # both coded: only the coded rows are uploaded; they become coded records [tpos, f0, mel-cepstrum, bands] on the
        # device and one call synthesises from them (world_hip_synthesis_records, wire 2)
        block = torch.cat([torch.zeros((n, 1), dtype=torch.float64, device=wh.device),
                           torch.from_numpy(read[1]).to(wh.device)[:, None], torch.from_numpy(sp).to(wh.device),
                           torch.from_numpy(ap).to(wh.device)], dim=1).contiguous()
        y = wh.synthesize_records(block, [n], fs, fft_size, frame_period, [y_length], wire=2, number_of_dimensions=sp.shape[1])
        wh.wavwrite(a.o, y[0, :y_length], fs)
        print(f"{n} frames -> {a.o} ({y_length} samples at {fs} Hz)")
        return
    f0 = torch.from_numpy(read[1]).to(wh.device)[None]
    sp, ap = torch.from_numpy(sp).to(wh.device)[None], torch.from_numpy(ap).to(wh.device)[None]
    if int(files.header(a.sp, "NOD ")):
        sp = wh.decode_spectral_envelope(sp, fs, fft_size)
    if int(files.header(a.ap, "NOD ")):
        ap = wh.decode_aperiodicity(ap, fs, fft_size)
    y = wh.synthesis(f0, sp, ap, np.array([n], dtype=np.int32), fft_size, frame_period, fs,
                     np.array([y_length], dtype=np.int32))
    wh.wavwrite(a.o, y[0, :y_length], fs)
    print(f"{n} frames -> {a.o} ({y_length} samples at {fs} Hz)")


def _load_batch(wh, chunk):
    """WAV files of one sampling rate -> (x [B, L] on the device, x_len): PCM bytes up, FP64 made on the device"""
    import torch
    waves = [wh.wavread(path)[0] for path in chunk]
    x = torch.zeros((len(chunk), max(w.numel() for w in waves)), dtype=torch.float64, device=wh.device)
    for row, w in enumerate(waves):
        x[row, :w.numel()] = w
    return x, np.array([w.numel() for w in waves], dtype=np.int32)


def _same_file(a, b):
    if os.path.realpath(a) == os.path.realpath(b):
        return True
    try:
        return os.path.samefile(a, b)                       # (hard links)
    except OSError:
        return False


def transform_outputs(wavs, outdir):
    """The file `transform` writes for each input: outdir/<the input's name>.  Refused, before anything is read or
    written, when an output would be one of the inputs or two inputs would share an output."""
    outs = [os.path.join(outdir, os.path.basename(path)) for path in wavs]
    seen = {}
    for path, out in zip(wavs, outs):
        key = os.path.realpath(out)
        if key in seen:
            raise ValueError(f"{path} and {seen[key]} would both be written to {out}")
        seen[key] = path
        for src in wavs:
            if _same_file(out, src):
                raise ValueError(f"{out} is an input file: choose an --outdir that holds none of the inputs")
    return outs


def _transform(a):
    _check_rate("transform", a)
    try:
        outs = transform_outputs(a.wav, a.outdir)
    except ValueError as e:
        sys.exit(f"transform: {e}")
    if a.align_to is not None and (a.duration is not None or a.time_scale != 1.0):
        sys.exit("transform: --align-to takes its duration from the other recording; --duration and --time-scale cannot be "
                 "combined with it")
    # the per-frame route; without these options, exactly as before
    frames = a.duration is not None or a.f0_from is not None or a.align_to is not None
    if a.duration is not None and not a.duration * 1000.0 / a.s >= 1.0:
        sys.exit(f"transform: --duration {a.duration} is shorter than one frame shift")
    track = None
    if a.f0_from is not None:
        read = FileAPI().read_f0(a.f0_from)
        if read is None or len(read[1]) < 1:
            sys.exit(f"transform: {a.f0_from} is not a readable F0 file")
        track = read[1]
    wh = WorldHip()
    a.other = None                                              # --align-to: the other recording, analysed once (_align_to)
    if a.align_to is not None:
        try:
            a.other = dict(fs=wh.wav_layout(a.align_to)[0])
        except Exception as e:
            sys.exit(f"transform: --align-to {a.align_to} is not a readable WAV file ({e})")
    os.makedirs(a.outdir, exist_ok=True)
    out_of = dict(zip(a.wav, outs))
    by_rate = {}
    for path in a.wav:
        by_rate.setdefault(wh.wav_layout(path)[0], []).append(path)
    samples = 0
    for src_fs, group in sorted(by_rate.items()):
        for at in range(0, len(group), a.batch):
            chunk = group[at:at + a.batch]
            x, x_len = _load_batch(wh, chunk)
            try:
                x, x_len, fs = _at_rate(wh, x, x_len, src_fs, a.fs, a.quality)
            except ValueError as e:
                sys.exit(f"transform: {e}")
            if frames:
                y, y_len = _resynthesize_frames(wh, a, x, fs, x_len, track)
            else:
                y, y_len = wh.resynthesize(x, fs, x_len=x_len, f0_scale=a.f0_scale, formant_shift=a.formant_shift,
                                           time_scale=a.time_scale, frame_period=a.s, f0_floor=a.f, f0_ceil=a.c)
            q = wh.double_to_pcm16(y).cpu().numpy()              # quantised on the device: int16 crosses PCIe
            for row, path in enumerate(chunk):
                n, name = int(y_len[row]), out_of[path]
                pcm = np.ascontiguousarray(q[row, :n])
                if wh.lib.world_hip_wav_write_pcm16(os.fsencode(name), fs, n, pcm.ctypes.data) != 1:
                    sys.exit(f"transform: {name} cannot be written")
                samples += n
    print(f"{len(a.wav)} file(s), {samples} samples -> {a.outdir}")


def _resynthesize_frames(wh, a, x, fs, x_len, track):
    """--duration / --f0-from: every utterance spread over its output frames by a uniform time map (--duration seconds, or
    its own length times --time-scale), the F0 file's track spread over the same frames as the target F0"""
    import torch
    n_src = [frame_count(fs, int(n), a.s) for n in x_len]
    aligned = None
    if a.align_to is not None:
        aligned = _align_to(wh, a, x, fs, x_len)
        n_out = [aligned.shape[1]] * len(n_src)
    elif a.duration is not None:
        n_out = [int(a.duration * 1000.0 / a.s) + 1] * len(n_src)
    else:
        n_out = [max(int((n - 1) * a.time_scale) + 1, 2) for n in n_src]
    O = max(n_out)
    time_map = torch.zeros((len(n_src), O), dtype=torch.float64, device=wh.device)
    for row, (n, m) in enumerate(zip(n_src, n_out)):
        time_map[row, :m] = uniform_time_map(n, m, device=wh.device) if aligned is None else aligned[row]
    f0_target = None
    if track is not None:
        src = torch.from_numpy(np.ascontiguousarray(track, dtype=np.float64)).to(wh.device)[None].contiguous()
        f0_target = torch.zeros_like(time_map)
        for m in sorted(set(n_out)):                              # (the track between two of its frames: modify_frames' F0 rules)
            spread = wh.modify_frames(src, None, None, [len(track)], fs, cheaptrick_fft_size(fs, 71.0),
                                      time_map=uniform_time_map(len(track), m, device=wh.device))[0][0]
            for row in (r for r, k in enumerate(n_out) if k == m):
                f0_target[row, :m] = spread
    return wh.resynthesize_frames(x, fs, x_len=x_len, n_out=n_out, time_map=time_map, f0_target=f0_target,
                                  f0_scale=a.f0_scale, formant_shift=a.formant_shift, frame_period=a.s, f0_floor=a.f,
                                  f0_ceil=a.c)


ALIGN_DIMS = 25       # mel-cepstral coefficients the alignments are made from (c0 is left out unless asked for)


def _coded_block(wh, x, fs, x_len, frame_period, dims, f0_floor=71.0, f0_ceil=800.0):
    """analyze_coded of one batch -> (block [rows, cols], first row of every utterance, frames of every utterance)"""
    import torch
    nf = np.array([frame_count(fs, int(n), frame_period) for n in x_len], dtype=np.int64)
    cols = wh.lib.world_hip_coded_columns(fs, dims)
    block = torch.zeros((int(nf.sum()), cols), dtype=torch.float64, device=wh.device)
    wh.analyze_coded(x, fs, block, x_len=x_len, frame_period=frame_period, f0_floor=f0_floor, f0_ceil=f0_ceil,
                     number_of_dimensions=dims)
    return block, np.concatenate([[0], np.cumsum(nf)[:-1]]), nf


def _cepstra(block, dims, keep_c0):
    return block[:, 2:2 + dims] if keep_c0 else block[:, 3:2 + dims]


def _align_to(wh, a, x, fs, x_len):
    """--align-to: the time map [B, n_other] that gives every input the timing of the other recording -- the mid-points
    of the DTW path between the input's and the other's mel-cepstra, per frame of the other"""
    if a.other["fs"] != fs and a.fs is None:
        sys.exit(f"transform: {a.align_to} has another sampling rate ({a.other['fs']} Hz) than the {fs} Hz inputs")
    if "block" not in a.other:                                  # (once for all batches: they all arrive at one rate -- their
        other, other_len = _load_batch(wh, [a.align_to])        #  own, the other's, or with --fs any source rates at F)
        try:
            other, other_len, _ = _at_rate(wh, other, other_len, a.other["fs"], a.fs, a.quality)
        except ValueError as e:
            sys.exit(f"transform: --align-to {a.align_to}: {e}")
        a.other["block"], a.other["row"], a.other["nf"] = _coded_block(wh, other, fs, other_len, a.s, ALIGN_DIMS, a.f, a.c)
    blk_b, row_b, nf_b = a.other["block"], a.other["row"], a.other["nf"]
    blk_a, row_a, nf_a = _coded_block(wh, x, fs, x_len, a.s, ALIGN_DIMS, a.f, a.c)
    B = len(nf_a)
    _, _, _, map_b, _ = wh.align(_cepstra(blk_a, ALIGN_DIMS, False), _cepstra(blk_b, ALIGN_DIMS, False), nf_a,
                                 np.repeat(nf_b, B), a_row=row_a, b_row=np.repeat(row_b, B), want_path=False)
    return map_b


def _mcep_block(wh, x, fs, x_len, frame_period, order, alpha):
    """_coded_block with all-pass mel-cepstra: analyze, then sp2mc of every utterance's frames straight into columns
    2 .. 2 + order of coded-style records [0, 0, c0 .. c_order] -> (block, first row, frames)"""
    import torch
    _, _, sp, _, nf = wh.analyze(x, fs, x_len=x_len, frame_period=frame_period)
    nf = np.asarray(nf, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(nf)[:-1]])
    block = torch.zeros((int(nf.sum()), 2 + order + 1), dtype=torch.float64, device=wh.device)
    alpha = wh.mcep_alpha(fs) if alpha is None else alpha
    try:
        for u, (r, n) in enumerate(zip(first, nf)):
            wh.sp2mc(sp[u, :int(n)], order, alpha, out=block[int(r):int(r) + int(n), 2:])
    except RuntimeError as e:                                   # the library's refusal of an order or an alpha
        raise ValueError(str(e)) from None
    return block, first, nf


def mcd_pairs(wh, pairs, dims=ALIGN_DIMS, keep_c0=False, frame_period=5.0, batch=64, fs=None, quality="best", mcep=None,
              alpha=None):
    """[(ref.wav, test.wav)] -> [(frames of ref, frames of test, path length, MCD in dB)]: every file analysed once into
    coded records (batches per sampling rate), every pair aligned on the device, one align call per rate.  fs: every file
    is converted to that rate on the device first (batches per source rate), and pairs of any two rates can be scored.
    mcep: the features are the all-pass mel-cepstra c0 .. c_mcep (alpha: world_hip_mcep_alpha of the rate unless given)
    instead of `dims` coefficients of the reference's coder"""
    if mcep is not None:
        dims = mcep + 1
    target = fs
    by_source, rate_of = {}, {}
    for path in dict.fromkeys(p for pair in pairs for p in pair):
        source = wh.wav_layout(path)[0]
        rate_of[path] = source if target is None else target
        by_source.setdefault(source, []).append(path)
    for ref, test in pairs:
        if rate_of[ref] != rate_of[test]:
            raise ValueError(f"{ref} and {test} have different sampling rates")
    by_rate = {}                                                # analysis rate -> [(source rate, its files)]
    for source, group in sorted(by_source.items()):
        by_rate.setdefault(source if target is None else target, []).append((source, group))
    out = {}
    for fs, sources in sorted(by_rate.items()):
        import torch
        blocks, where, at = [], {}, 0
        for source, group in sources:
            for lo in range(0, len(group), batch):
                chunk = group[lo:lo + batch]
                x, x_len = _load_batch(wh, chunk)
                x, x_len, _ = _at_rate(wh, x, x_len, source, target, quality)
                if mcep is None:
                    block, first, nf = _coded_block(wh, x, fs, x_len, frame_period, dims)
                else:
                    block, first, nf = _mcep_block(wh, x, fs, x_len, frame_period, mcep, alpha)
                blocks.append(block)
                for path, r, n in zip(chunk, first, nf):
                    where[path] = (at + int(r), int(n))
                at += block.shape[0]
        block = torch.cat(blocks) if len(blocks) > 1 else blocks[0]
        mine = [pr for pr in pairs if rate_of[pr[0]] == fs]
        feats = _cepstra(block, dims, keep_c0)
        _, path_len, summary, _, _ = wh.align(feats, feats, [where[r][1] for r, _ in mine], [where[t][1] for _, t in mine],
                                              a_row=[where[r][0] for r, _ in mine], b_row=[where[t][0] for _, t in mine],
                                              want_path=False)
        summary = summary.cpu().numpy()
        for u, pr in enumerate(mine):
            out[pr] = (where[pr[0]][1], where[pr[1]][1], int(summary[u, 1]), float(summary[u, 2]))
    return [out[pr] for pr in pairs]


def _mcd(a):
    _check_rate("mcd", a)
    if len(a.wav) % 2:
        sys.exit("mcd: the files come in pairs: REF.wav TEST.wav [REF2.wav TEST2.wav ...]")
    if a.dims < (1 if a.keep_c0 else 2):
        sys.exit(f"mcd: --dims {a.dims} leaves no coefficient to compare")
    if a.mcep is not None and a.mcep < (0 if a.keep_c0 else 1):
        sys.exit(f"mcd: --mcep {a.mcep} leaves no coefficient to compare")
    pairs = list(zip(a.wav[0::2], a.wav[1::2]))
    try:
        results = mcd_pairs(WorldHip(), pairs, a.dims, a.keep_c0, a.s, a.batch, a.fs, a.quality, a.mcep, a.alpha)
    except ValueError as e:
        sys.exit(f"mcd: {e}")
    for (ref, test), (na, nb, K, mcd) in zip(pairs, results):
        print(f"{ref} {test}: frames {na} {nb} path {K} mcd {mcd:.6f} dB")


def morph_waves(wh, xa, xb, fs, rate=0.5, time_rate=None, f0_rate=None, sp_rate=None, ap_rate=None, fade=False,
                frame_period=5.0, f0_floor=71.0, f0_ceil=800.0):
    """Two waveforms (1-D float64 device tensors of one sampling rate) -> (y [1, Y], Y): both analysed, their envelopes
    coded to ALIGN_DIMS mel-cepstra and aligned without c0, the frames between them morphed and synthesised at the analysis
    frame period.  fade: the three feature rates rise linearly from 0 to 1 over the output.  Nothing but the two inputs
    and the output crosses the bus."""
    import torch
    fft_size = cheaptrick_fft_size(fs, 71.0)
    sides = []
    for x in (xa, xb):
        _, f0, sp, ap, nf = wh.analyze(x[None].contiguous(), fs, frame_period=frame_period, f0_floor=f0_floor, f0_ceil=f0_ceil)
        sides.append(((f0, sp, ap), nf, wh.code_spectral_envelope(sp, fs, fft_size, ALIGN_DIMS)))
    (a, nf_a, mc_a), (b, nf_b, mc_b) = sides
    path, path_len, _, _, _ = wh.align(mc_a[:, :, 1:], mc_b[:, :, 1:], nf_a, nf_b)
    time_rate = rate if time_rate is None else time_rate
    n_out = wh.morph_length(int(nf_a[0]), int(nf_b[0]), time_rate)
    if n_out < 2:
        raise ValueError(f"the morph has {n_out} frame(s); synthesis needs 2")
    if fade:
        f0_rate = sp_rate = ap_rate = torch.linspace(0.0, 1.0, n_out, dtype=torch.float64, device=wh.device)
    f0, sp, ap, no = wh.morph(a, b, nf_a, nf_b, fs, fft_size, path, path_len, rate=rate, time_rate=time_rate, f0_rate=f0_rate,
                              sp_rate=sp_rate, ap_rate=ap_rate)
    y_len = wh.resynthesis_length(fs, n_out, frame_period)
    return wh.synthesis(f0, sp, ap, no, fft_size, frame_period, fs, np.array([y_len], dtype=np.int32)), y_len


def _morph(a):
    for name in ("rate", "time_rate", "f0_rate", "sp_rate", "ap_rate"):
        v = getattr(a, name)
        if v is not None and not 0.0 <= v <= 1.0:
            sys.exit(f"morph: --{name.replace('_', '-')} {v} outside [0, 1]")
    if a.fade and (a.f0_rate is not None or a.sp_rate is not None or a.ap_rate is not None):
        sys.exit("morph: --fade sets the F0, envelope and aperiodicity rates itself")
    wh = WorldHip()
    try:
        (fs_a, fs_b) = (wh.wav_layout(path)[0] for path in (a.a, a.b))
    except Exception as e:
        sys.exit(f"morph: not a readable WAV file ({e})")
    if fs_a != fs_b and a.fs is None:
        sys.exit(f"morph: {a.b} has another sampling rate ({fs_b} Hz) than {a.a} ({fs_a} Hz)")
    xa, xb = wh.wavread(a.a)[0], wh.wavread(a.b)[0]
    fs = fs_a if a.fs is None else a.fs
    try:
        (xa, xb) = (_at_rate(wh, x[None].contiguous(), None, src, a.fs, a.quality)[0][0] for x, src in ((xa, fs_a), (xb, fs_b)))
    except ValueError as e:
        sys.exit(f"morph: {e}")
    try:
        y, y_len = morph_waves(wh, xa, xb, fs, a.rate, a.time_rate, a.f0_rate, a.sp_rate, a.ap_rate, a.fade, a.s, a.f, a.c)
    except ValueError as e:
        sys.exit(f"morph: {e}")
    wh.wavwrite(a.o, y[0, :y_len], fs)
    print(f"{a.a} {a.b} -> {a.o} ({y_len} samples at {fs} Hz)")


def _resample(a):
    _check_rate("resample", a)
    try:
        outs = transform_outputs(a.wav, a.outdir)
    except ValueError as e:
        sys.exit(f"resample: {e}")
    wh = WorldHip()
    by_rate = {}
    try:
        for path in a.wav:
            by_rate.setdefault(wh.wav_layout(path)[0], []).append(path)
    except OSError as e:
        sys.exit(f"resample: not a readable WAV file ({e})")
    os.makedirs(a.outdir, exist_ok=True)
    out_of = dict(zip(a.wav, outs))
    samples = 0
    for src_fs, group in sorted(by_rate.items()):
        for at in range(0, len(group), a.batch):
            chunk = group[at:at + a.batch]
            x, x_len = _load_batch(wh, chunk)
            try:
                y, y_len, _ = _at_rate(wh, x, x_len, src_fs, a.fs, a.quality)
            except ValueError as e:
                sys.exit(f"resample: {e}")
            q = wh.double_to_pcm16(y).cpu().numpy()              # quantised on the device: int16 crosses PCIe
            for row, path in enumerate(chunk):
                n, name = int(y_len[row]), out_of[path]
                pcm = np.ascontiguousarray(q[row, :n])
                if wh.lib.world_hip_wav_write_pcm16(os.fsencode(name), a.fs, n, pcm.ctypes.data) != 1:
                    sys.exit(f"resample: {name} cannot be written")
                samples += n
    print(f"{len(a.wav)} file(s), {samples} samples at {a.fs} Hz -> {a.outdir}")

UNVOICED_LF0 = -1e10  # .lf0 of an unvoiced frame (the HTS / Merlin convention)


def _features(a):
    _check_rate("features", a)
    if a.order < 0:
        sys.exit(f"features: --order {a.order}")
    wh = WorldHip()
    by_rate = {}
    try:
        for path in a.wav:
            by_rate.setdefault(wh.wav_layout(path)[0], []).append(path)
    except OSError as e:
        sys.exit(f"features: not a readable WAV file ({e})")
    os.makedirs(a.outdir, exist_ok=True)
    frames = 0
    for src_fs, group in sorted(by_rate.items()):
        for at in range(0, len(group), a.batch):
            chunk = group[at:at + a.batch]
            x, x_len = _load_batch(wh, chunk)
            try:
                x, x_len, fs = _at_rate(wh, x, x_len, src_fs, a.fs, a.quality)
                _, f0, sp, ap, nf = wh.analyze(x, fs, x_len=x_len, f0_method=a.f0, frame_period=a.s, f0_floor=a.f, f0_ceil=a.c)
                fft_size = cheaptrick_fft_size(fs, 71.0)
                alpha = wh.mcep_alpha(fs) if a.alpha is None else a.alpha
                mgc = wh.sp2mc(sp, a.order, alpha).cpu().numpy()
                bap = wh.code_aperiodicity(ap, fs, fft_size).cpu().numpy()
            except (ValueError, RuntimeError) as e:
                sys.exit(f"features: {e}")
            f0 = f0.cpu().numpy()
            for row, path in enumerate(chunk):
                n, stem = int(nf[row]), os.path.join(a.outdir, os.path.splitext(os.path.basename(path))[0])
                voiced = f0[row, :n] > 0
                lf0 = np.where(voiced, np.log(np.where(voiced, f0[row, :n], 1.0)), UNVOICED_LF0)
                for ext, v in ((".lf0", lf0), (".mgc", mgc[row, :n]), (".bap", bap[row, :n])):
                    np.ascontiguousarray(v).astype("<f4").tofile(stem + ext)
                frames += n
    print(f"{len(a.wav)} file(s), {frames} frames -> {a.outdir}")


def _features_synthesis(a):
    import torch
    wh = WorldHip()
    if a.fs < 1 or a.order < 0:
        sys.exit(f"features-synthesis: --fs {a.fs} --order {a.order}")
    try:
        lf0, mgc, bap = (np.fromfile(path, dtype="<f4").astype(np.float64) for path in (a.lf0, a.mgc, a.bap))
    except OSError as e:
        sys.exit(f"features-synthesis: {e}")
    n, nap = lf0.size, wh.lib.GetNumberOfAperiodicities(a.fs)
    if n < 1 or mgc.size != n * (a.order + 1) or nap < 1 or bap.size != n * nap:
        sys.exit(f"features-synthesis: {n} frames of ln F0, but {mgc.size} values of {a.order + 1} mel-cepstra and {bap.size} "
                 f"of {nap} band aperiodicities")
    fft_size = cheaptrick_fft_size(a.fs, 71.0)
    f0 = np.where(lf0 > 0.5 * UNVOICED_LF0, np.exp(np.where(lf0 > 0.5 * UNVOICED_LF0, lf0, 0.0)), 0.0)
    try:
        alpha = wh.mcep_alpha(a.fs) if a.alpha is None else a.alpha
        sp = wh.mc2sp(torch.from_numpy(mgc.reshape(n, a.order + 1)).to(wh.device), alpha, fft_size)
        ap = wh.decode_aperiodicity(torch.from_numpy(bap.reshape(n, nap)).to(wh.device), a.fs, fft_size)
        y_length = int(n * a.s / 1000.0 * a.fs)
        y = wh.synthesis(torch.from_numpy(f0).to(wh.device)[None], sp[None], ap[None], np.array([n], dtype=np.int32), fft_size,
                         a.s, a.fs, np.array([y_length], dtype=np.int32))
    except (ValueError, RuntimeError) as e:
        sys.exit(f"features-synthesis: {e}")
    wh.wavwrite(a.o, y[0, :y_length], a.fs)
    print(f"{n} frames -> {a.o} ({y_length} samples at {a.fs} Hz)")


def _float_rows(tool, path, cols):
    """a headerless float32 file of rows of `cols` values -> float64 [rows][cols]"""
    try:
        v = np.fromfile(path, dtype="<f4").astype(np.float64)
    except OSError as e:
        sys.exit(f"{tool}: {e}")
    if v.size < cols or v.size % cols:
        sys.exit(f"{tool}: {path} holds {v.size} values, no positive multiple of {cols}")
    return v.reshape(-1, cols)


def _deltas(a):
    import torch
    dim = 1 if a.lf0 and a.dim is None else a.dim
    if dim is None or dim < 1:
        sys.exit(f"deltas: --dim {dim}")
    x = _float_rows("deltas", a.x, dim)
    wh = WorldHip()
    try:
        d_x = torch.from_numpy(x).to(wh.device)
        mask = (d_x[:, 0] > 0.5 * UNVOICED_LF0) if a.lf0 else None
        out = wh.deltas(d_x, mask=mask, fill=UNVOICED_LF0 if a.lf0 else 0.0)
    except (ValueError, RuntimeError) as e:
        sys.exit(f"deltas: {e}")
    out.cpu().numpy().astype("<f4").tofile(a.o)
    print(f"{len(x)} frames of {dim} -> {a.o} ([{len(x)}][{out.shape[1]}])")


def _mlpg(a):
    import torch
    dim = 1 if a.lf0 and a.dim is None else a.dim
    if dim is None or dim < 1:
        sys.exit(f"mlpg: --dim {dim}")
    n_win = len(WorldHip.DEFAULT_WINDOWS)
    mean, var = _float_rows("mlpg", a.mean, n_win * dim), _float_rows("mlpg", a.var, n_win * dim)
    if len(var) not in (1, len(mean)):
        sys.exit(f"mlpg: {len(mean)} rows of means but {len(var)} of variances (as many, or one)")
    wh = WorldHip()
    try:
        d_mean, d_var = torch.from_numpy(mean).to(wh.device), torch.from_numpy(var).to(wh.device)
        mask = (d_mean[:, 0] > 0.5 * UNVOICED_LF0) if a.lf0 else None
        out = wh.mlpg(d_mean, d_var, mask=mask, precision=a.precision, fill=UNVOICED_LF0 if a.lf0 else 0.0)
    except (ValueError, RuntimeError) as e:
        sys.exit(f"mlpg: {e}")
    out.cpu().numpy().astype("<f4").tofile(a.o)
    print(f"{len(mean)} frames of {n_win} x {dim} -> {a.o} ([{len(mean)}][{dim}])")


VC_WINDOWS = WorldHip.DEFAULT_WINDOWS[:2]   # the conversion model sees [static, delta]


def vc_speaker(wh, utterances):
    """one speaker's utterances, a list of statics [T][D] (float64 on the device) -> (statics [P][F][D] padded with zeros,
    [static, delta] [P][F][2 D] of the whole utterances in one deltas call, the frame counts [P] int32)"""
    import torch
    n = np.array([len(x) for x in utterances], dtype=np.int32)
    statics = torch.zeros((len(utterances), int(n.max()), int(utterances[0].shape[1])), dtype=torch.float64, device=wh.device)
    for u, x in enumerate(utterances):
        statics[u, :len(x)] = x
    dyn = torch.zeros((statics.shape[0], statics.shape[1], 2 * statics.shape[2]), dtype=torch.float64, device=wh.device)
    wh.deltas(statics, windows=VC_WINDOWS, n_frames=n, out=dyn)
    return statics, dyn, n


def vc_power_gate(wh, statics, n, fs, gate_db, alpha=None, batch=16):
    """the frames of each utterance whose power is at least 10^(gate_db / 10) times the utterance's mean: the envelope of the
    mel-cepstra (mc2sp at the rate's all-pass constant and CheapTrick's default fft_size) -> frame_power -> select_frames.
    -> (index [P][F] int32, count [P] int32 on the host)"""
    import torch
    fft_size = cheaptrick_fft_size(fs)
    alpha = wh.mcep_alpha(fs) if alpha is None else alpha
    index, count = [], []
    for u0 in range(0, len(n), batch):
        block, nb = statics[u0:u0 + batch], n[u0:u0 + batch]
        sp = wh.mc2sp(block.reshape(-1, block.shape[2]), alpha, fft_size).reshape(block.shape[0], block.shape[1], -1)
        power, mean = wh.frame_power(sp, nb)
        i, c, _ = wh.select_frames(power, nb, 10.0 ** (gate_db / 10.0), scale=mean)
        index.append(i)
        count.append(c)
    return torch.cat(index), torch.cat(count).cpu().numpy()


def vc_joint_rows(wh, a, b, gate_a=None, gate_b=None, align_a=None):
    """every pair at once: a, b = vc_speaker()'s triples of the two speakers -> (the joint rows [x, dx, y, dy] along the DTW
    paths of the statics without c0, [sum of the path lengths][4 D]; each pair's MCD along its path in dB, on the host).
    gate_a / gate_b: vc_power_gate()'s (index, count): alignment and rows use the kept frames only (the deltas are those of
    the whole utterance).  align_a: statics to align in the source's place (a realignment's converted ones); the rows are
    the source's own either way.  One align call, one host read (the path lengths), one joint_rows call."""
    (sa, xa, na), (sb, xb, nb) = a, b
    sa = sa if align_a is None else align_a
    fa, fb, ca, cb = sa[:, :, 1:], sb[:, :, 1:], na, nb
    if gate_a is not None:
        fa, ca = wh.gather_rows(fa, gate_a[0], gate_a[1], n_src=na), gate_a[1]
    if gate_b is not None:
        fb, cb = wh.gather_rows(fb, gate_b[0], gate_b[1], n_src=nb), gate_b[1]
    path, path_len, summary, _, _ = wh.align(fa, fb, ca, cb)
    z = wh.joint_rows(xa, xb, path, path_len, sel_a=None if gate_a is None else gate_a[0], sel_b=None if gate_b is None else gate_b[0],
                      n_a=na, n_b=nb, n_sel_a=None if gate_a is None else gate_a[1], n_sel_b=None if gate_b is None else gate_b[1])
    return z, summary[:, 2].cpu().numpy()


def vc_convert_statics(wh, w, mu, cov, speaker):
    """a speaker's utterances through the model: gmm_convert (the mixture) on [static, delta], then mlpg -> statics [P][F][D]"""
    _, dyn, n = speaker
    model = wh.gmm_prepare(w, mu, cov, dyn.shape[2])
    mean, var = wh.gmm_convert(model, dyn.reshape(-1, dyn.shape[2]))
    return wh.mlpg(mean.reshape(dyn.shape), var.reshape(dyn.shape), windows=VC_WINDOWS, n_frames=n)


def _vc_train(a):
    import torch
    if a.dim < 2 or a.mix < 1 or a.iter < 1 or len(a.src) != len(a.target):
        sys.exit(f"vc-train: --dim {a.dim} (at least 2: c0 and one more), --mix {a.mix}, --iter {a.iter}, {len(a.src)} source and "
                 f"{len(a.target)} target files (as many of each)")
    if a.realign < 0 or (a.power_gate is not None and (a.fs is None or a.fs < 1)):
        sys.exit(f"vc-train: --realign {a.realign} (0 or more); --power-gate needs --fs, the sampling rate the .mgc files were made at")
    wh = WorldHip()
    try:
        load = lambda files: vc_speaker(wh, [torch.from_numpy(_float_rows("vc-train", f, a.dim)).to(wh.device) for f in files])
        src, tgt = load(a.src), load(a.target)
        gates = [None, None]
        if a.power_gate is not None:
            gates = [vc_power_gate(wh, s[0], s[2], a.fs, a.power_gate) for s in (src, tgt)]
            for g, s, name in zip(gates, (src, tgt), ("source", "target")):
                if int(g[1].min()) < 1:
                    sys.exit(f"vc-train: --power-gate {a.power_gate} dB keeps no frame of {name} file {int(g[1].argmin()) + 1}")
                print(f"{name}: {int(g[1].sum())} of {int(s[2].sum())} frames at or above {a.power_gate} dB of their utterance's mean power")
        z, mcd = vc_joint_rows(wh, src, tgt, *gates)
        w, mu, cov, loglik = wh.gmm_fit(z, a.mix, n_iter=a.iter, reg=a.reg)
        for r in range(a.realign):
            print(f"round {r}: {len(z)} joint rows, mean log-likelihood {loglik[-1]:.4f}, mean MCD along the paths {mcd.mean():.4f} dB")
            z, mcd = vc_joint_rows(wh, src, tgt, *gates, align_a=vc_convert_statics(wh, w, mu, cov, src))
            w, mu, cov, loglik = wh.gmm_fit(z, a.mix, n_iter=a.iter, reg=a.reg, init=(w, mu, cov))
        if a.realign:
            print(f"round {a.realign}: {len(z)} joint rows, mean log-likelihood {loglik[-1]:.4f}, mean MCD along the paths {mcd.mean():.4f} dB")
    except (ValueError, RuntimeError) as e:
        sys.exit(f"vc-train: {e}")
    np.savez(a.o, w=w, mu=mu, cov=cov, dim=np.int64(a.dim), dx=np.int64(2 * a.dim), loglik=loglik)
    print(f"{len(a.src)} pair(s), {len(z)} joint rows of {z.shape[1]} -> {a.o} ({a.mix} mixtures; mean log-likelihood "
          f"{loglik[0]:.4f} -> {loglik[-1]:.4f})")


def _vc_convert(a):
    import torch
    try:
        with np.load(a.model) as f:
            w, mu, cov, dim, dx = f["w"], f["mu"], f["cov"], int(f["dim"]), int(f["dx"])
    except (OSError, KeyError, ValueError) as e:
        sys.exit(f"vc-convert: {a.model}: {e}")
    if a.dim != dim:
        sys.exit(f"vc-convert: --dim {a.dim}, but the model was trained on {dim} values per frame")
    x = _float_rows("vc-convert", a.mgc, dim)
    wh = WorldHip()
    try:
        model = wh.gmm_prepare(w, mu, cov, dx)
        mean, var = wh.gmm_convert(model, wh.deltas(torch.from_numpy(x).to(wh.device), windows=VC_WINDOWS), mode=a.mode)
        out = wh.mlpg(mean, var, windows=VC_WINDOWS)
    except (ValueError, RuntimeError) as e:
        sys.exit(f"vc-convert: {e}")
    out.cpu().numpy().astype("<f4").tofile(a.o)
    print(f"{len(x)} frames of {dim} -> {a.o}")


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m world_amd.tools", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="tool", required=True)
    an = sub.add_parser("analysis", help="WAV files -> .f0 / .sp / .ap files")
    an.add_argument("wav", nargs="+")
    an.add_argument("--outdir", default=".")
    an.add_argument("--f0", choices=("harvest", "dio"), default="harvest", help="dio = Dio + StoneMask")
    an.add_argument("-f", type=float, default=71.0, help="floor of the F0 range (Hz)")
    an.add_argument("-c", type=float, default=800.0, help="ceiling of the F0 range (Hz)")
    an.add_argument("-s", type=float, default=5.0, help="frame shift (ms)")
    an.add_argument("-q", type=float, default=-0.15, help="CheapTrick q1")
    an.add_argument("-t", type=float, default=0.85, help="D4C threshold")
    an.add_argument("--text", action="store_true", help="write .f0 as text")
    an.add_argument("--code-sp", type=int, default=0, metavar="D", help="store D mel-cepstral coefficients per frame")
    an.add_argument("--code-ap", action="store_true", help="store band aperiodicities")
    an.add_argument("--batch", type=int, default=64, help="utterances per GPU call")
    an.set_defaults(run=_analysis)
    sy = sub.add_parser("synthesis", help=".f0 + .sp + .ap -> WAV")
    sy.add_argument("f0")
    sy.add_argument("sp")
    sy.add_argument("ap")
    sy.add_argument("-o", default="output.wav")
    sy.set_defaults(run=_synthesis)
    tr = sub.add_parser("transform", help="WAV files -> analysed, modified and resynthesised WAV files")
    tr.add_argument("wav", nargs="+")
    tr.add_argument("--outdir", required=True, help="written under the input files' names; must hold none of the inputs")
    tr.add_argument("--f0-scale", type=float, default=1.0, help="F0 multiplier (test.cpp's third argument)")
    tr.add_argument("--formant-shift", type=float, default=1.0, help="spectral envelope stretch (test.cpp's fourth argument)")
    tr.add_argument("--time-scale", type=float, default=1.0, help="duration multiplier (synthesis frame period * T)")
    tr.add_argument("--duration", type=float, default=None, metavar="SECONDS",
                    help="every output lasts SECONDS: the frames are spread by a uniform time map (replaces --time-scale)")
    tr.add_argument("--f0-from", default=None, metavar="FILE.f0",
                    help="voiced frames take their F0 from this F0 file's track, spread over the output frames")
    tr.add_argument("--align-to", default=None, metavar="OTHER.wav",
                    help="every output takes OTHER's timing: the time map is the DTW alignment of the input to OTHER, one "
                         "output frame per frame of OTHER (composes with --f0-from)")
    tr.add_argument("-f", type=float, default=71.0, help="floor of the F0 range (Hz)")
    tr.add_argument("-c", type=float, default=800.0, help="ceiling of the F0 range (Hz)")
    tr.add_argument("-s", type=float, default=5.0, help="frame shift of the analysis (ms)")
    tr.add_argument("--batch", type=int, default=64, help="utterances per GPU call")
    tr.set_defaults(run=_transform)
    mc = sub.add_parser("mcd", help="pairs of WAV files -> mel-cepstral distortion along the DTW path")
    mc.add_argument("wav", nargs="+", metavar="REF.wav TEST.wav")
    mc.add_argument("--dims", type=int, default=ALIGN_DIMS, help="mel-cepstral coefficients per frame, c0 included")
    mc.add_argument("--keep-c0", action="store_true", help="compare c0 too (by default the energy term is left out)")
    mc.add_argument("-s", type=float, default=5.0, help="frame shift of the analysis (ms)")
    mc.add_argument("--batch", type=int, default=64, help="utterances per GPU call")
    mc.set_defaults(run=_mcd)
    mo = sub.add_parser("morph", help="two WAV files -> the utterance between them")
    mo.add_argument("a", metavar="A.wav")
    mo.add_argument("b", metavar="B.wav")
    mo.add_argument("-o", default="morph.wav")
    mo.add_argument("--rate", type=float, default=0.5, help="0 = A, 1 = B: the rate of everything not given a rate of its own")
    mo.add_argument("--time-rate", type=float, default=None, help="timing: part-way along the alignment of A and B")
    mo.add_argument("--f0-rate", type=float, default=None, help="F0 (geometric)")
    mo.add_argument("--sp-rate", type=float, default=None, help="spectral envelope (geometric)")
    mo.add_argument("--ap-rate", type=float, default=None, help="aperiodicity (linear)")
    mo.add_argument("--fade", action="store_true", help="F0, envelope and aperiodicity go from A to B over the output")
    mo.add_argument("-f", type=float, default=71.0, help="floor of the F0 range (Hz)")
    mo.add_argument("-c", type=float, default=800.0, help="ceiling of the F0 range (Hz)")
    mo.add_argument("-s", type=float, default=5.0, help="frame shift of the analysis (ms)")
    mo.set_defaults(run=_morph)
    rs = sub.add_parser("resample", help="WAV files -> WAV files of one sampling rate")
    rs.add_argument("wav", nargs="+")
    rs.add_argument("--outdir", required=True, help="written under the input files' names; must hold none of the inputs")
    rs.add_argument("--fs", type=int, required=True, metavar="F", help="the sampling rate of every output (Hz)")
    rs.add_argument("--quality", choices=("best", "fast"), default="best", help="the filter: 64 or 16 zero crossings a side")
    rs.add_argument("--batch", type=int, default=64, help="utterances per GPU call")
    rs.set_defaults(run=_resample)
    mc.add_argument("--mcep", type=int, default=None, metavar="M",
                    help="score the all-pass mel-cepstra c1 .. cM (sp2mc) instead of --dims coefficients of the reference's coder")
    mc.add_argument("--alpha", type=float, default=None, help="the all-pass constant of --mcep (default: the rate's)")
    fe = sub.add_parser("features", help="WAV files -> .lf0 / .mgc / .bap files (float32)")
    fe.add_argument("wav", nargs="+")
    fe.add_argument("--outdir", default=".")
    fe.add_argument("--order", type=int, required=True, metavar="M", help="mel-cepstra c0 .. cM per frame")
    fe.add_argument("--alpha", type=float, default=None, help="the all-pass constant (default: the rate's, 0.41 at 16 kHz)")
    fe.add_argument("--f0", choices=("harvest", "dio"), default="harvest", help="dio = Dio + StoneMask")
    fe.add_argument("-f", type=float, default=71.0, help="floor of the F0 range (Hz)")
    fe.add_argument("-c", type=float, default=800.0, help="ceiling of the F0 range (Hz)")
    fe.add_argument("-s", type=float, default=5.0, help="frame shift (ms)")
    fe.add_argument("--batch", type=int, default=64, help="utterances per GPU call")
    fe.set_defaults(run=_features)
    fs_ = sub.add_parser("features-synthesis", help=".lf0 + .mgc + .bap -> WAV")
    fs_.add_argument("lf0")
    fs_.add_argument("mgc")
    fs_.add_argument("bap")
    fs_.add_argument("--fs", type=int, required=True, metavar="F", help="the sampling rate the features were made at (Hz)")
    fs_.add_argument("--order", type=int, required=True, metavar="M")
    fs_.add_argument("--alpha", type=float, default=None, help="the all-pass constant (default: the rate's)")
    fs_.add_argument("-s", type=float, default=5.0, help="frame shift (ms)")
    fs_.add_argument("-o", default="output.wav")
    fs_.set_defaults(run=_features_synthesis)
    de = sub.add_parser("deltas", help="[frames][dim] float32 statics -> [frames][3 dim]: static, delta, delta-delta")
    de.add_argument("x", metavar="X")
    de.add_argument("--dim", type=int, default=None, metavar="D", help="values per frame (with --lf0: 1)")
    de.add_argument("--lf0", action="store_true", help="-1e10 marks unvoiced frames: masked, and -1e10 in the output")
    de.add_argument("-o", required=True)
    de.set_defaults(run=_deltas)
    ml = sub.add_parser("mlpg", help="[frames][3 dim] means + variances ([frames] or 1 row) -> the [frames][dim] trajectory")
    ml.add_argument("mean", metavar="MEAN")
    ml.add_argument("var", metavar="VAR")
    ml.add_argument("--dim", type=int, default=None, metavar="D", help="static values per frame (with --lf0: 1)")
    ml.add_argument("--lf0", action="store_true", help="frames whose static mean is -1e10 are masked and stay -1e10")
    ml.add_argument("--precision", action="store_true", help="VAR holds 1 / variance")
    ml.add_argument("-o", required=True)
    ml.set_defaults(run=_mlpg)
    vt = sub.add_parser("vc-train", help="pairs of .mgc files of two speakers -> a joint-density Gaussian mixture (model.npz)")
    vt.add_argument("src", nargs="+", metavar="SRC.mgc")
    vt.add_argument("--target", nargs="+", required=True, metavar="TGT.mgc", help="the other speaker's files, in the same order")
    vt.add_argument("--dim", type=int, required=True, metavar="D", help="values per frame (order + 1)")
    vt.add_argument("--mix", type=int, default=32, metavar="M", help="mixtures")
    vt.add_argument("--iter", type=int, default=20, metavar="N", help="EM iterations")
    vt.add_argument("--reg", type=float, default=1e-6, help="added to the diagonal of every covariance")
    vt.add_argument("--power-gate", type=float, default=None, metavar="DB",
                    help="align and train on the frames whose power is at least DB dB of their utterance's mean (-20: the usual "
                         "silence gate), each speaker by itself; needs --fs")
    vt.add_argument("--fs", type=int, default=None, metavar="F", help="the sampling rate the .mgc files were made at (Hz)")
    vt.add_argument("--realign", type=int, default=0, metavar="R",
                    help="R times: convert the sources with the fitted model, align the converted frames to the targets, refit")
    vt.add_argument("-o", required=True, metavar="model.npz")
    vt.set_defaults(run=_vc_train)
    vc = sub.add_parser("vc-convert", help="a model and a source .mgc -> the converted .mgc (deltas, conversion, MLPG)")
    vc.add_argument("model", metavar="model.npz")
    vc.add_argument("mgc", metavar="A.mgc")
    vc.add_argument("--dim", type=int, required=True, metavar="D")
    vc.add_argument("--mode", choices=("mixture", "hard"), default="mixture", help="hard: the most likely component alone")
    vc.add_argument("-o", required=True)
    vc.set_defaults(run=_vc_convert)
    for tool in (an, tr, mc, mo, fe):
        tool.add_argument("--fs", type=int, default=None, metavar="F",
                          help="convert every input whose sampling rate differs from F to F on the device first")
        tool.add_argument("--quality", choices=("best", "fast"), default="best", help="the filter of that conversion")
    a = p.parse_args(argv)
    a.run(a)


if __name__ == "__main__":
    main()
