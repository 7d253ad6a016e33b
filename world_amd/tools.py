"""Batch command-line tools over the reference's file formats.

The reference ships one-file-at-a-time programs (examples/parameter_io/f0analysis.cpp,
spanalysis.cpp, apanalysis.cpp, readandsynthesis.cpp); these do the same work for MANY files
per call, batched on the GPU, and read / write the same F0 / SPEC / AP / WAV files:

    python -m world_amd.tools analysis a.wav b.wav ... --outdir params      # -> params/a.f0 a.sp a.ap ...
    python -m world_amd.tools synthesis params/a.f0 params/a.sp params/a.ap -o a_resynth.wav
    python -m world_amd.tools transform a.wav b.wav ... --outdir out --f0-scale 1.5 --formant-shift 1.2
    python -m world_amd.tools transform a.wav --outdir out --duration 2.5 --f0-from melody.f0

`analysis` keeps the example programs' option letters where they exist (-f/-c/-s of f0analysis,
-q of spanalysis, -t of apanalysis).  Files are grouped by sampling rate; only their PCM bytes
are uploaded (decoded on the device), and with --code-sp / --code-ap the envelopes are coded on
the device before they come back, so the D2H traffic and the files shrink by 10-17x.
`transform` is the reference test program's analysis -> ParameterModification -> Synthesis (F0 scale, formant shift,
and a speed change through the synthesis frame period) in one library call per batch; the waveforms are quantised to
16 bits on the device, so only int16 samples come back.  With --duration or --f0-from the modification is per frame
(world_hip_resynthesize_frames_batch): a uniform time map to the asked length, and the F0 track of another file as target.
There is no CPU path: without a GPU and the built library this exits with an error.
"""
import argparse
import os
import sys

import numpy as np

from .api import FileAPI, WorldHip, cheaptrick_fft_size, frame_count, uniform_time_map


def _analysis(a):
    wh, files = WorldHip(), FileAPI()
    os.makedirs(a.outdir, exist_ok=True)
    by_rate = {}
    for path in a.wav:
        by_rate.setdefault(wh.wav_layout(path)[0], []).append(path)
    frames = 0
    for fs, group in sorted(by_rate.items()):
        for at in range(0, len(group), a.batch):
            chunk = group[at:at + a.batch]
            x, x_len = _load_batch(wh, chunk)
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
    try:
        outs = transform_outputs(a.wav, a.outdir)
    except ValueError as e:
        sys.exit(f"transform: {e}")
    frames = a.duration is not None or a.f0_from is not None    # the per-frame route; without them, exactly as before
    if a.duration is not None and not a.duration * 1000.0 / a.s >= 1.0:
        sys.exit(f"transform: --duration {a.duration} is shorter than one frame shift")
    track = None
    if a.f0_from is not None:
        read = FileAPI().read_f0(a.f0_from)
        if read is None or len(read[1]) < 1:
            sys.exit(f"transform: {a.f0_from} is not a readable F0 file")
        track = read[1]
    wh = WorldHip()
    os.makedirs(a.outdir, exist_ok=True)
    out_of = dict(zip(a.wav, outs))
    by_rate = {}
    for path in a.wav:
        by_rate.setdefault(wh.wav_layout(path)[0], []).append(path)
    samples = 0
    for fs, group in sorted(by_rate.items()):
        for at in range(0, len(group), a.batch):
            chunk = group[at:at + a.batch]
            x, x_len = _load_batch(wh, chunk)
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
    if a.duration is not None:
        n_out = [int(a.duration * 1000.0 / a.s) + 1] * len(n_src)
    else:
        n_out = [max(int((n - 1) * a.time_scale) + 1, 2) for n in n_src]
    O = max(n_out)
    time_map = torch.zeros((len(n_src), O), dtype=torch.float64, device=wh.device)
    for row, (n, m) in enumerate(zip(n_src, n_out)):
        time_map[row, :m] = uniform_time_map(n, m, device=wh.device)
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
    tr.add_argument("-f", type=float, default=71.0, help="floor of the F0 range (Hz)")
    tr.add_argument("-c", type=float, default=800.0, help="ceiling of the F0 range (Hz)")
    tr.add_argument("-s", type=float, default=5.0, help="frame shift of the analysis (ms)")
    tr.add_argument("--batch", type=int, default=64, help="utterances per GPU call")
    tr.set_defaults(run=_transform)
    a = p.parse_args(argv)
    a.run(a)


if __name__ == "__main__":
    main()
