"""``locate()``: find when given words are spoken without transcribing the whole recording.

Behavioural contract = ``stable_whisper/alignment.py::locate`` (:756-1116).  Per 30-s chunk:

1. one teacher-forced pass over ``initial_tokens + text_tokens`` with the alignment heads' cross-attention captured; the
   frame where the LAST text token attends most (after softmax over frames, z-normalisation over tokens, median-7 and
   the head mean -- the same processing as the word-timestamp path, but over every token row) approximates where the
   text ends (:930-951);
2. (modes 0, 1) the ``duration_window`` seconds around that time are decoded greedily, token by token, while the search
   text is forced in whenever it is likely enough (probability, exact arg-max, or string match) (:975-1065);
3. (mode 0) the decoded tokens get word timestamps against the whole chunk (:1089-1107).

Device work goes through four engine calls that exist for the hot path anyway: log-mel + encoder + cross-KV, the scoring
pass (``engine.score`` with no row cropping: ``n_sot = 0``), and ``engine.forward_logits``.  The greedy loop is host
logic with one logits call per token (<= ``max_token_per_seg`` + 1 tokens).  It mirrors the reference's bookkeeping
exactly, including what its KV cache holds after a partly matched text is rolled back (:1040-1048: the cache is cleared
and decoding continues from the single next token) -- observable behaviour, so it is kept.  Checked against the
reference's ``locate`` on the CPU oracle through the engine stand-in (tests/test_locate_cpu.py).
"""
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from .stabilization import host_single_thread
from .audio import FRAMES_PER_SECOND, N_FFT, N_FRAMES, N_SAMPLES, SAMPLE_RATE
from .decoding import DecodingOptions, DecodingPlan
from .result import Segment
from .timing import add_word_timestamps_batch, split_word_tokens

CHUNK_LENGTH = N_SAMPLES // SAMPLE_RATE


def _chunk_mel(model, audio_segment: torch.Tensor) -> torch.Tensor:
    """log-mel [n_mels, 3000] of one chunk as the reference computes it for locate (:924-925): the segment plus
    N_FFT // 2 + 1 zero samples, trimmed / zero-filled to 3000 frames (swx_log_mel_ragged)."""
    return model.log_mel_segments([audio_segment], padding=N_FFT // 2 + 1)[0]


def _pad_frames(mel: torch.Tensor) -> torch.Tensor:
    out = torch.zeros(mel.shape[0], N_FRAMES, dtype=mel.dtype, device=mel.device)
    k = min(N_FRAMES, mel.shape[-1])
    out[:, :k] = mel[:, :k]
    return out


def next_token_on_host(row: torch.Tensor, eot: int, suppressed: List[int], target: int) -> tuple:
    """The answer to a next-token query from one logits row ``[eot + 1]`` (f32, host), with the reference's arithmetic
    (:995-1010): suppressed ids at -inf, the two last entries of an ascending sort, softmax over ``[:eot]``.  Returns ``(best,
    runner_up, p_target, p_best, p_runner_up)``; a probability is 0.0 where the id is not below ``eot`` (target -1)."""
    row[suppressed] = -np.inf
    top2 = row.sort(dim=-1).indices[-2:]
    best, runner_up = int(top2[-1]), int(top2[-2])
    probs = row[:eot].softmax(dim=-1)
    p = [probs[t].item() if 0 <= t < eot else 0.0 for t in (best, runner_up)]
    return best, runner_up, (0.0 if target == -1 else probs[target].item()), p[0], p[1]


class LocateJob:
    """Everything ``locate`` settles before it touches the audio, and the per-recording state machine (``steps``).  The state
    machine is host logic only: it yields a request wherever a device call is made and receives the answer, so that one driver
    can answer the requests of one recording with batch-1 calls (``locate``) and another those of many recordings with one call
    per phase (``many.locate_many``).  Requests:

    * ``("chunk", samples)`` -> a handle of the chunk's log-mel and cross-K/V;
    * ``("end_row", handle, tokens)`` -> f32 host ``[n_audio_ctx]``: the last token's row of the alignment matrix;
    * ``("section", handle, frame0, frame1)`` -> a handle of the cross-K/V of these mel frames, zero-padded to 30 s;
    * ``("next", section handle, tokens, target id or -1)`` -> ``(best, runner_up, p_target, p_best, p_runner_up)``;
    * ``("words", handle, tokens, num_samples)`` -> the word dicts of ``add_word_timestamps_batch``."""

    def __init__(self, model, text: Union[str, List[int]], language: str, count: int = 1,
                 duration_window: Union[float, Tuple[float, float]] = 3.0, *, mode: int = 0, start: float = None,
                 end: float = None, probability_threshold: float = 0.5, eots: int = 1, max_token_per_seg: int = 20,
                 exact_token: bool = False, case_sensitive: bool = False, verbose: Optional[bool] = False,
                 initial_prompt: str = None, suppress_tokens: Union[str, List[int]] = "-1", **unsupported):
        from .transcribe import pop_audio_options
        self.audio_options = pop_audio_options(unsupported)
        if unsupported:
            raise TypeError(f"locate() got unexpected keyword argument(s): {sorted(unsupported)}")
        self.sec_per_emb = model.dims.n_audio_ctx / CHUNK_LENGTH
        self.n_audio_ctx = model.dims.n_audio_ctx
        if isinstance(duration_window, (float, int)):
            duration_window = [duration_window] * 2
        assert N_SAMPLES > sum(duration_window), f"Sum of [duration_window] must be less than {N_SAMPLES}, got {sum(duration_window)}"
        self.duration_window = duration_window
        self.adjusted_chunk = N_SAMPLES - round(duration_window[0] * SAMPLE_RATE)
        if initial_prompt:
            initial_prompt = " " + initial_prompt.strip()
        plan = DecodingPlan(model, DecodingOptions(language=language, prompt=initial_prompt, suppress_tokens=suppress_tokens,
                                                   without_timestamps=True))
        self.tok = tok = plan.tokenizer
        self.initial_tokens = list(plan.initial_tokens)
        self.text_tokens, text = (tok.encode(text), text) if isinstance(text, str) else (list(text), tok.decode(list(text)))
        if not exact_token and not case_sensitive:
            text = text.lower()
        self.text = text
        self.suppressed = [t for t in plan.suppress if t < tok.eot]
        self.count, self.mode, self.start, self.end = count, mode, start, end
        self.probability_threshold, self.eots, self.max_token_per_seg = probability_threshold, eots, max_token_per_seg
        self.exact_token, self.case_sensitive, self.verbose = exact_token, case_sensitive, verbose

    def waveform(self, audio) -> torch.Tensor:
        from .transcribe import as_waveform
        return as_waveform(audio, **self.audio_options).detach().float().cpu()

    def steps(self, audio: torch.Tensor):
        """generator over the requests of one recording (``audio``: what ``waveform`` returned); returns the matches"""
        tok, mode, count = self.tok, self.mode, self.count
        initial_tokens, text_tokens, text = self.initial_tokens, self.text_tokens, self.text
        duration_window, probability_threshold = self.duration_window, self.probability_threshold
        exact_token, case_sensitive, eots, max_token_per_seg = self.exact_token, self.case_sensitive, self.eots, self.max_token_per_seg
        if self.end:
            audio = audio[:round(self.end * SAMPLE_RATE)]
        seek_sample = round(self.start * SAMPLE_RATE) if self.start else 0
        total = int(audio.shape[-1])
        found = 0
        prev_target_end = None
        matches = []

        while seek_sample < total and (not count or found < count):
            seek = round(seek_sample / SAMPLE_RATE, 3)
            chunk = audio[seek_sample: seek_sample + N_SAMPLES]
            whole = yield ("chunk", chunk)
            # -- 1. where does the text end?  alignment matrix over every row of initial_tokens + text_tokens
            last_row = yield ("end_row", whole, initial_tokens + text_tokens)
            target_end = round((last_row.argmax() / self.sec_per_emb).item(), 3)
            if mode == 2:
                found += 1
                if seek_sample + N_SAMPLES >= total or (count and found >= count) or prev_target_end == target_end:
                    seek_sample = total
                else:
                    seek_sample += round(target_end * SAMPLE_RATE)
                prev_target_end = target_end
                matches.append(dict(tokens=[], target_end=target_end + seek))
                continue
            # -- 2. greedy decode of the duration window with the search text forced in
            curr_start = round(max(target_end - duration_window[0], 0.0), 3)
            curr_end = round(target_end + duration_window[1], 3)
            section = yield ("section", whole, round(curr_start * FRAMES_PER_SECOND), round(curr_end * FRAMES_PER_SECOND))
            cache: List[int] = []                    # what the reference's KV cache holds = the context of the next logits
            feed: List[int] = list(initial_tokens)   # `temp_tokens`: what is appended to the cache by the next call
            fed_log: List[List[int]] = [list(initial_tokens)]      # `infer_tokens`
            predictions = []
            target_idx = 0
            running, found_target = True, False
            curr_eots = 0
            to_decode: List[int] = []
            replaced: List[int] = []
            while running:
                cache = cache + feed
                best, runner_up, p_target, p_best, p_runner_up = yield ("next", section, list(cache),
                                                                        -1 if found_target else text_tokens[target_idx])
                best_non_eot = runner_up if best == tok.eot else best
                p_non_eot = p_runner_up if best == tok.eot else p_best
                # The reference keeps `best_token` / `best_non_eot_token` as views of one small tensor: when the arg-max is
                # not EOT they are the SAME element, so forcing the target token in place (:1022) also rewrites the copy that
                # was just queued for string matching and the value compared two lines later.  `same_slot` carries that.
                same_slot = best != tok.eot
                queued = False
                if found_target:
                    target_prob = is_match = None
                else:
                    if exact_token:
                        is_match = False
                    else:
                        to_decode.append(best_non_eot)
                        queued = True
                        temp_text = tok.decode(to_decode)
                        if not case_sensitive:
                            temp_text = temp_text.lower()
                        is_match = temp_text.endswith(text)
                        if is_match:
                            to_decode = []
                            queued = False
                    target_prob = p_target
                if target_prob is not None and (target_prob >= probability_threshold or
                                                best_non_eot == text_tokens[target_idx] or is_match):
                    if is_match:
                        best = best_non_eot
                        token_prob = p_non_eot
                        found_target = True
                    else:
                        best = text_tokens[target_idx]
                        if same_slot:
                            best_non_eot = best
                            if queued:
                                to_decode[-1] = best
                        if replaced or best_non_eot != text_tokens[target_idx]:
                            replaced.append(best_non_eot)
                        target_idx += 1
                        if target_idx == len(text_tokens):
                            found_target = True
                        token_prob = target_prob
                    if found_target:
                        found += 1
                    curr_eots = 0
                else:
                    if not found_target:
                        if replaced:
                            # :1040-1046 rebuilds the decoder input with torch.cat of a [1, n - k] and a [1, k] tensor along
                            # dim 0, which only works for n - k == k; the same call is made here so that the same error
                            # surfaces.  The rebuilt input is then overwritten below; what remains is the cleared cache.
                            n_fed = sum(len(x) for x in fed_log)
                            torch.cat([torch.zeros(1, n_fed - len(replaced), dtype=torch.long),
                                       torch.zeros(1, len(replaced), dtype=torch.long)])
                            replaced = []
                            cache = []
                        target_idx = 0
                    if best == tok.eot:
                        if curr_eots >= eots or found_target:
                            running = False
                        else:
                            curr_eots += 1
                            best = best_non_eot
                            p_best = p_non_eot
                    else:
                        curr_eots = 0
                    token_prob = None if best == tok.eot else p_best
                predictions.append(dict(token=best, prob=token_prob))
                if len(predictions) > max_token_per_seg:
                    running = False
                if running:
                    fed_log.append([best])
                    feed = [best]
            match = None
            if found_target:
                final_tokens = [p["token"] for p in predictions]
                if mode == 1:
                    _, (ws, wts), _ = split_word_tokens([dict(tokens=final_tokens)], tok)
                    tprobs = [p["prob"] for p in predictions]
                    wps = [float(np.mean([tprobs.pop(0) for _ in wt])) for wt in wts]
                    words = [dict(word=w, tokens=wt, probability=wp) for w, wt, wp in zip(ws, wts, wps)]
                    match = dict(end=target_end + seek, text=text, duration_window_text="".join(ws), duration_window_word=words)
                    seek_sample += round(curr_end * SAMPLE_RATE)
                else:
                    words = yield ("words", whole, final_tokens, round(curr_end * SAMPLE_RATE))
                    match = Segment(words=words)
                    seek_sample += round(match.words[-1].end * SAMPLE_RATE)
                    match.offset_time(seek)
                    match.seek = curr_start
                if self.verbose:
                    print(f'Confirmed: "{text}" ending at ~{target_end + seek:.3f}s')
            else:
                seek_sample += self.adjusted_chunk if chunk.shape[-1] == N_SAMPLES else int(chunk.shape[-1])
            if match:
                matches.append(match)
        if self.verbose and not matches:
            print(f'Failed to locate "{text}".')
        return matches


def end_row_tokens(job: LocateJob, seq: List[int]) -> List[int]:
    """the token row of the scoring pass that answers ``("end_row", handle, seq)``"""
    return seq + [job.tok.eot]


@host_single_thread
def locate(model, audio, text: Union[str, List[int]], language: str, count: int = 1,
           duration_window: Union[float, Tuple[float, float]] = 3.0, *, mode: int = 0, start: float = None,
           end: float = None, probability_threshold: float = 0.5, eots: int = 1, max_token_per_seg: int = 20,
           exact_token: bool = False, case_sensitive: bool = False, verbose: Optional[bool] = False,
           initial_prompt: str = None, suppress_tokens: Union[str, List[int]] = "-1", **unsupported):
    job = LocateJob(model, text, language, count, duration_window, mode=mode, start=start, end=end,
                    probability_threshold=probability_threshold, eots=eots, max_token_per_seg=max_token_per_seg,
                    exact_token=exact_token, case_sensitive=case_sensitive, verbose=verbose, initial_prompt=initial_prompt,
                    suppress_tokens=suppress_tokens, **unsupported)
    tok, eng = job.tok, model.engine
    steps = job.steps(job.waveform(audio))
    got = None
    while True:
        try:
            request = steps.send(got)
        except StopIteration as done:
            return done.value
        kind = request[0]
        if kind == "chunk":
            mel = _chunk_mel(model, request[1])
            got = dict(mel=mel, xkv=model.cross_kv(model.encoder(mel[None])))
        elif kind == "end_row":
            seq = request[2]
            _, neg, _ = eng.score(request[1]["xkv"], [end_row_tokens(job, seq)], [model.dims.n_audio_ctx], n_sot=0, eot=tok.eot)
            got = (-neg[0, len(seq) - 1, : model.dims.n_audio_ctx]).float().cpu()
        elif kind == "section":
            section = _pad_frames(request[1]["mel"][..., request[2]: request[3]])
            got = model.cross_kv(model.encoder(section[None]))
        elif kind == "next":
            seq = request[2]
            row = eng.forward_logits(request[1], [seq])[0, len(seq) - 1, : tok.eot + 1].float().cpu().clone()
            got = next_token_on_host(row, tok.eot, job.suppressed, request[3])
        else:
            seg = dict(seek=0, tokens=request[2])
            add_word_timestamps_batch(model=model, tokenizer=tok, xkv=request[1]["xkv"], gap_padding=None,
                                      windows=[dict(segments=[seg], num_samples=request[3])])
            got = seg["words"]
