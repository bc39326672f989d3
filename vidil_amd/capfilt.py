"""Frame captioning + CapFilt filtering driver — the hot loop of the reference's
run_video_CapFilt.py (:93-126 helpers, :139-204 ``CapFilt``, :206-291 ``main``).

``caption_frames`` / ``filter_captions`` keep the reference's per-video call shapes.
``CapFiltEngine`` is the batched, de-duplicated schedule the throughput path uses:
many videos per launch, ViT once per frame per model, cross-attention K/V once per
frame, all (frame, caption) pairs of the batch through the ITM encoder in one pass,
one device->host copy per batch.  Frame decoding/sampling (decord) stays outside:
the engine takes already-sampled uint8 frames (parity is defined on given frames).
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import dist as vdist
from .blip import CLIP_MEAN, CLIP_STD, blip_decoder
from .blip_itm import blip_itm
from .preprocess import blip_frames


@torch.no_grad()
def caption_frames(captioner, images, mode="beam"):
    """run_video_CapFilt.py:93-105."""
    if mode == "beam":
        return captioner.generate(images, sample=False, num_beams=3, max_length=20, min_length=5)
    return captioner.generate(images, sample=True, top_p=0.9, max_length=20, min_length=5)


def keep_caption(itm_score, threshold, mode="max_filter"):
    """run_video_CapFilt.py:116-123 on the per-frame match probabilities of one caption."""
    s = np.asarray(itm_score, dtype=np.float32)
    prob = np.sum(s) / len(s) if mode == "avg_filter" else np.max(s)
    return bool(prob > threshold)


@torch.no_grad()
def filter_captions(filterer, images, texts, threshold, mode="max_filter"):
    """run_video_CapFilt.py:107-126, reference call shape (one filterer call per caption)."""
    kept = []
    for t in texts:
        itm_output = filterer(images, [t for _ in range(images.size()[0])], match_head="itm")
        itm_score = torch.nn.functional.softmax(itm_output, dim=1)[:, 1].detach().cpu().numpy()
        if keep_caption(itm_score, threshold, mode):
            kept.append(t)
    return kept


@torch.no_grad()
def score_captions(captioner, images, texts, label_smoothing=0.0):
    """The captioner's own likelihood of ``texts`` on every frame, beside the ITM probability of ``filter_captions``:
    images f32 [F,3,S,S], C texts WITHOUT the prompt (what ``caption_frames`` returns, or original captions) -> f32 [C, F]
    of negative log-likelihood per scored token (lower: more likely).  The ViT runs once per frame and all C*F pairs go
    through one teacher-forced pass, image-major (BLIP_Decoder.caption_nll / BertLMHeadModel.score)."""
    F, texts = images.shape[0], list(texts)
    C = len(texts)
    _, y16 = captioner.visual_encoder.forward_both(images)
    nll, count = captioner.caption_nll(y16.view(F, -1, y16.shape[-1]), texts * F, group_start=torch.arange(F + 1) * C,
                                       add_prompt=True, label_smoothing=label_smoothing, reduction="none")
    return (nll / count.clamp(min=1)).view(F, C).t().contiguous()


def dedup(captions):
    """run_video_CapFilt.py:185-188."""
    out = []
    for c in captions:
        if c not in out:
            out.append(c)
    return out


def split_sentences(texts, do_sentence_tokenization=True):
    """run_video_CapFilt.py:166-175: spaCy ``doc.sents`` of every original caption.

    Without spaCy (or its ``en_core_web_sm`` model) the sentence boundaries — hence which original-caption sentences
    become candidates — would differ from the reference, so that is an error unless the plain '. ' splitter is
    requested explicitly with VIDIL_SENTENCE_SPLIT=naive (a one-time warning is printed then)."""
    if not texts:
        return []
    if not do_sentence_tokenization:
        return [t.replace("\n", ". ").strip() for t in texts]
    nlp = sentence_splitter()
    out = []
    for t in texts:
        for sent in sentences_of(nlp, t.replace("\n", ". ")):
            if len(sent) > 3:
                out.append(sent.strip())
    return out


def sentences_of(nlp, text):
    """The sentence texts of ``text`` under a splitter: a spaCy pipeline (``doc.sents``) or "naive" (plain '. ' splitting)."""
    if nlp == "naive":
        return text.split(". ")
    return [sent.text for sent in nlp(text).sents]


def sentence_splitter():
    """The splitter ``split_sentences`` uses, loaded once: spaCy's en_core_web_sm, or "naive" when that is missing and
    VIDIL_SENTENCE_SPLIT=naive asks for it (anything else raises)."""
    nlp = split_sentences.__dict__.get("_nlp")
    if nlp is None:
        try:
            import spacy

            nlp = spacy.load("en_core_web_sm", disable=["ner", "tagger", "lemmatizer"])
        except (ImportError, OSError) as e:
            if os.environ.get("VIDIL_SENTENCE_SPLIT", "") != "naive":
                raise RuntimeError(
                    "do_sentence_tokenization needs spaCy with en_core_web_sm (as the reference, run_video_CapFilt.py:"
                    "166-175); set VIDIL_SENTENCE_SPLIT=naive to accept plain '. ' splitting instead, or "
                    "do_sentence_tokenization: false") from e
            import warnings

            warnings.warn("vidil_amd.capfilt: spaCy/en_core_web_sm not available; splitting original captions on '. ' "
                          "(VIDIL_SENTENCE_SPLIT=naive) — sentence boundaries may differ from the reference")
            nlp = "naive"
        split_sentences._nlp = nlp
    return nlp


_REQUIRED_KEYS = ("caption", "filter")


def validate_config(cfg):
    """The reference indexes its YAML directly (run_video_CapFilt.py:141-204): a missing key is a KeyError there, and
    some combinations cannot work.  Check up front instead of defaulting silently."""
    for k in _REQUIRED_KEYS:
        if k not in cfg:
            raise KeyError(f"CapFilt config lacks '{k}' (the reference's pipeline YAMLs set it)")
    if cfg["filter"]:
        for k in ("threshold", "filter_generated_only"):
            if k not in cfg:
                raise KeyError(f"CapFilt config lacks '{k}' (required when filter is on)")
    if cfg["caption"] and "keep_original_caption" not in cfg:
        raise KeyError("CapFilt config lacks 'keep_original_caption' (required when caption is on)")
    if cfg["filter"] and not cfg["caption"] and cfg["filter_generated_only"]:
        raise ValueError("caption=False with filter=True and filter_generated_only=True filters an empty list and keeps "
                         "every original caption unfiltered; set filter_generated_only=False to filter the originals")
    if cfg.get("filter_mode", "max_filter") not in ("max_filter", "avg_filter"):
        raise ValueError(f"unknown filter_mode {cfg['filter_mode']!r}")


class CapFiltEngine:
    """Batched CapFilt over already-sampled frames.

    config keys (configs/pipeline_config/*.yaml of the reference): caption, filter,
    filter_generated_only, keep_original_caption, threshold, filter_mode, generation_mode,
    do_sentence_tokenization, image_size, vit, caption_model_ckpt, filterer_model_ckpt.
    Own keys: tower_chunk_videos (round 6: the ViTs, the CLIP tower and the ITM run over at most this many videos at a time while
    ONE beam search runs over every image of the batch — the decode steps' GEMMs have 3 rows per image, so a search over the
    images of several tower chunks runs them at 4x the rows per launch; 0 / absent = no chunking); itm_chunk_videos (the ITM passes
    over at most this many videos — default: the tower chunk; their per-image cross K/V are sized by it); decode_streams (parts of the batch whose beam searches run side by side on their own streams; default 1:
    measured +0.2 % with 2, -4 % with 4 at 3,072 frames — a decode step already occupies the chip); itm_short_circuit (default False = score every (frame, caption) pair like the reference; True = the
    any()-short-circuit of ``_filter_enqueue``, same kept lists with a fraction of the ITM work).
    """

    def __init__(self, config, device, captioner=None, filterer=None):
        validate_config(config)
        self.config = config
        self.device = torch.device(device)
        S, vit = config.get("image_size", 224), config.get("vit", "base")
        if captioner is None:
            captioner = blip_decoder(pretrained=config.get("caption_model_ckpt", ""), image_size=S, vit=vit)
        if filterer is None:
            filterer = blip_itm(pretrained=config.get("filterer_model_ckpt", ""), image_size=S, vit=vit)
        self.captioner = captioner.eval().to(self.device)
        self.filterer = filterer.eval().to(self.device)
        self.last_stats = {}
        self.last_frame_captions = []
        self._pinned = {}

    @torch.no_grad()
    def process(self, items, frames_u8):
        """items: list of dicts {'video_id', 'text': [original captions]}; frames_u8: uint8 [Nv,F,H,W,3]
        device tensor (any H x W: resized to S x S like ``process_frame``, run_video_CapFilt.py:128-134).
        Fills item['text'] / item['unfiltered_text'] like run_video_CapFilt.py:166-204.

        The four phases below are public so a caller can put other GPU work between them (vidil_amd.pipeline does, with
        the CLIP visual tokens): the host only ever waits on an event recorded right after the results it needs, while
        the queue behind that event already holds the next tower."""
        st = self.begin(items, frames_u8)
        self.encode_filter_frames(st)
        self.captions_ready(st)
        return self.finish(st)

    def _to_host(self, key, t):
        """Enqueue a device->pinned-host copy of ``t`` and an event behind it; returns (host tensor, event)."""
        buf = self._pinned.get(key)
        if buf is None or buf.shape != t.shape or buf.dtype != t.dtype:
            buf = self._pinned[key] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        buf.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return buf, ev

    @torch.no_grad()
    def begin(self, items, frames_u8):
        """Phase 1 (no host wait): resize, caption ViT, the whole beam / nucleus decode, token ids on their way to the host."""
        cfg = self.config
        Nv, F = frames_u8.shape[0], frames_u8.shape[1]
        st = dict(items=items, Nv=Nv, F=F, tok=None, fy16=None, itm=None)
        st["spans"] = spans = self.tower_spans(Nv)
        st["flat"] = flat = blip_frames(frames_u8.reshape(Nv * F, *frames_u8.shape[2:]), cfg.get("image_size", 224))
        if cfg["caption"]:
            # the caption ViT over one tower chunk at a time (its activations are sized by the chunk), every chunk's image tokens
            # into ONE beam search: a search is per image and every decode kernel's arithmetic is independent of the rows around
            # a row, so the captions are those of per-chunk searches (tests/test_models_gpu.py) at a multiple of the rows per launch
            ys = [self.captioner.visual_encoder.forward_u8(flat[a * F:b * F], CLIP_MEAN, CLIP_STD)[1] for a, b in spans]
            y16 = ys[0] if len(ys) == 1 else torch.cat(ys)
            del ys
            if cfg.get("generation_mode", "beam") == "beam":
                out_tok, _ = self.captioner.generate_ids(y16, Nv * F, num_beams=3, max_length=20, min_length=5,
                                                         streams=cfg.get("decode_streams", 1))
            else:   # nucleus sampling, run_video_CapFilt.py:103-104
                out_tok = self.captioner.sample_ids(y16, Nv * F, top_p=0.9, max_length=20, min_length=5,
                                                    seed=cfg.get("sample_seed"))
            st["tok"] = self._to_host("tok", out_tok)
        return st

    def tower_spans(self, Nv):
        """[start, end) video ranges the towers and the ITM run over (config ``tower_chunk_videos``; one span when unset)."""
        c = int(self.config.get("tower_chunk_videos") or 0)
        if c <= 0 or Nv <= c:
            return [(0, Nv)]
        return [(a, min(a + c, Nv)) for a in range(0, Nv, c)]

    @torch.no_grad()
    def encode_filter_frames(self, st):
        """Phase 2 (no host wait): the filter's ViT needs the frames only, so it is queued before the host blocks on the
        caption ids and runs while the captions are decoded to strings, de-duplicated and tokenised again."""
        if self.config["filter"]:
            F = st["F"]
            st["fy16"] = [self.filterer.visual_encoder.forward_u8(st["flat"][a * F:b * F], CLIP_MEAN, CLIP_STD)[1] for a, b in st["spans"]]

    @torch.no_grad()
    def captions_ready(self, st):
        """Phase 3: wait for the caption ids, build the candidate lists (reference branches at :177-195) and queue the
        ITM pairs; their probabilities start their way to the host."""
        cfg, items, Nv, F = self.config, st["items"], st["Nv"], st["F"]
        generated = [[] for _ in range(Nv)]
        if st["tok"] is not None:
            host_tok, ev = st["tok"]
            ev.synchronize()
            caps = self.captioner.decode_captions(host_tok)
            self.last_frame_captions = caps
            generated = [dedup(caps[v * F:(v + 1) * F]) for v in range(Nv)]
            # the first frame each distinct caption came from (itm_short_circuit scores a caption there first)
            st["home"] = [{c: f for f, c in reversed(list(enumerate(caps[v * F:(v + 1) * F])))} for v in range(Nv)]
        to_filter = []
        for v, item in enumerate(items):
            orig = split_sentences(item.get("text", []), cfg.get("do_sentence_tokenization", True))
            if not cfg["caption"]:
                cand = orig
                item["unfiltered_text"] = cand
                gen = []
            else:
                gen = generated[v]
                if cfg["keep_original_caption"]:
                    cand = orig + gen
                else:
                    item["text"] = []
                    cand = gen
                item["unfiltered_text"] = cand
            if cfg["filter"]:
                to_filter.append(gen if cfg["filter_generated_only"] else cand)
            else:
                item["text"] = cand
                to_filter.append(None)
        st["generated"], st["to_filter"] = generated, to_filter
        if cfg["filter"]:
            # the ITM pairs of one tower chunk at a time (a video's pairs only meet that video's frames): the per-image cross K/V of
            # the filter are sized by the chunk and released behind the chunk's last launch
            home = st.get("home")
            st["itm"], st["itm_spans"] = [], []
            c_itm = int(cfg.get("itm_chunk_videos") or 0)     # (own key: ITM passes over fewer videos than a tower chunk — the filter's
            for (a, b), fy in zip(st["spans"], st["fy16"]):   #  per-image cross K/V, 8.3 MB per frame, are sized by THIS chunk)
                Te_rows = fy.shape[0] // (b - a)              # rows of the filter ViT's output per video (F x tokens per frame)
                subs = [(a, b)] if c_itm <= 0 or b - a <= c_itm else [(x, min(x + c_itm, b)) for x in range(a, b, c_itm)]
                for a2, b2 in subs:
                    many = len(st["spans"]) > 1 or len(subs) > 1
                    pend = self._filter_enqueue(fy[(a2 - a) * Te_rows:(b2 - a) * Te_rows], b2 - a2, F, to_filter[a2:b2],
                                                None if home is None else home[a2:b2], tag=f"{a2}:" if many else "")
                    if pend is not None and many:
                        pend["cross"] = None                   # (every launch that reads them is queued: stream-ordered reuse;
                        if not pend["short"]:                  #  the short circuit's second phase projects them again, _cross_of)
                            pend["y16"] = None
                    st["itm"].append(pend)
                    st["itm_spans"].append((a2, b2))
            st["fy16"] = None

    @torch.no_grad()
    def finish(self, st):
        """Phase 4: wait for the ITM probabilities, apply the threshold rule, fill the items."""
        cfg, items, Nv, F = self.config, st["items"], st["Nv"], st["F"]
        n_pairs = 0
        if cfg["filter"]:
            kept = []
            for (a, b), pend in zip(st["itm_spans"], st["itm"]):
                kept.extend(self._filter_finish(pend, b - a, F, st["to_filter"][a:b]))
                n_pairs += pend["n_pairs"] if pend is not None else 0
                if pend is not None and len(st["itm"]) > 1:
                    pend["cross"] = pend["y16"] = None
            for v, item in enumerate(items):
                if cfg["filter_generated_only"]:
                    item["text"] = list(item.get("text", [])) + kept[v]
                else:
                    item["text"] = kept[v]
        self.last_stats = dict(videos=Nv, frames=Nv * F, unique_captions=sum(len(g) for g in st["generated"]),
                               itm_pairs=n_pairs)
        return items

    # ------------------------------------------------------------------ the filter's text side
    # Candidate captions of the batch are numbered globally (video-major); a (caption, frame) pair is scored by at most
    # one ``itm_pairs`` call and lands in a dense [captions, F] probability matrix (NaN = never scored).  Calls differ
    # in WHICH pairs they hold — all of them, one length bucket, a short-circuit phase — never in what a pair's score is.

    #: upper token counts of the length buckets (CLS + words + SEP, models/blip_itm.py:46 pads everything to 35)
    LENGTH_EDGES = (8, 12, 16, 20, 24, 28, 35)
    #: a bucket with fewer pairs than this is merged into the next longer one (its GEMMs would not fill the chip)
    MIN_BUCKET_PAIRS = 2048
    #: ... unless merging a small TAIL bucket would pad the previous bucket's pairs by more rows than this
    MERGE_MAX_EXTRA_ROWS = 10_000

    def _length_buckets(self, cap_idx, lens_np, pairs_per_cap):
        """Split caption indices by token count so that a call's rows are cut to ITS longest caption (the reference pads
        to 35; itm_pairs already cuts a call to the longest caption in it).  Invisible when all captions have the same
        length; on real captions (10-14 tokens, a few long ones) it removes the padding rows of the short ones."""
        buckets, cur, cur_pairs = [], [], 0
        order = cap_idx[np.argsort(lens_np[cap_idx], kind="stable")]
        edge = 0
        for c in order:
            while lens_np[c] > self.LENGTH_EDGES[edge]:
                edge += 1
                if cur and cur_pairs >= self.MIN_BUCKET_PAIRS:
                    buckets.append(np.sort(np.asarray(cur)))
                    cur, cur_pairs = [], 0
            cur.append(c)
            cur_pairs += pairs_per_cap
        if cur:
            merge = False
            if buckets and cur_pairs < self.MIN_BUCKET_PAIRS:
                # a small tail (a few long captions among thousands) may join the previous bucket instead of paying a full
                # 12-layer launch sequence for a handful of rows — but that call is then cut to the TAIL's longest caption, so
                # every pair of the previous bucket is padded up to it: merge on a cost test, the rows the merge
                # adds against what a launch sequence is worth (~2 ms of launches ~ 10^4 rows of encoder work)
                prev = buckets[-1]
                extra_rows = len(prev) * pairs_per_cap * (int(lens_np[np.asarray(cur)].max()) - int(lens_np[prev].max()))
                merge = extra_rows <= self.MERGE_MAX_EXTRA_ROWS
            if merge:
                buckets[-1] = np.sort(np.concatenate([buckets[-1], np.asarray(cur)]))
            else:
                buckets.append(np.sort(np.asarray(cur)))   # (itm_pairs falls back to its small-call layout for a thin call: min_rows)
        return buckets

    def _cross_of(self, pend):
        """The filter's per-image cross K/V of this chunk — projected again if they were released after the chunk's first phase
        (the short circuit over several chunks: 8.3 MB per frame are not kept for every chunk of the batch until the second phase)."""
        if pend["cross"] is None:
            pend["cross"] = self.filterer.project_image_kv(pend["y16"], pend["n_images"], pend["min_rows"])
        return pend["cross"]

    def _score(self, pend, cap_idx, frame_of=None):
        """Queue the ITM of captions ``cap_idx`` (global indices, ascending) against the frames of their videos — all
        F, or only ``frame_of[c]`` when given (int array aligned with cap_idx).  Pair order is IMAGE-major (video, frame,
        caption) so the captions of a frame are consecutive and share one fetch of that frame's cross K/V; the
        reference's loop is caption-major (run_video_CapFilt.py:110-112) but a pair's score does not depend on the order."""
        F, flt = pend["F"], self.filterer
        vid = pend["cap_video"][cap_idx]
        sub = torch.from_numpy(cap_idx)
        ids, lens = pend["ids"].index_select(0, sub), pend["lens"].index_select(0, sub)
        local = np.arange(len(cap_idx), dtype=np.int64)
        if frame_of is not None:                      # one pair per caption: pair -> image map
            image = (vid * F + frame_of).astype(np.int32)
            logits = flt.itm_pairs(pend["y16"], pend["n_images"], ids, lens, image_index=torch.from_numpy(image),
                                   pair_text=torch.from_numpy(local), cross=self._cross_of(pend))
            pair_c, pair_f = cap_idx, np.asarray(frame_of, dtype=np.int64)
        else:
            skip = pend.get("skip")
            pair_c, pair_f, counts = [], [], np.zeros(pend["n_images"], dtype=np.int64)
            # captions are video-major, so the captions of one video are one run of cap_idx
            starts = np.flatnonzero(np.r_[True, vid[1:] != vid[:-1]])
            ends = np.r_[starts[1:], len(vid)]
            for a, b in zip(starts, ends):
                v = int(vid[a])
                run = local[a:b]
                for f in range(F):
                    here = run if skip is None else run[skip[cap_idx[a:b]] != f]
                    counts[v * F + f] = len(here)
                    pair_c.append(here)
                    pair_f.append(np.full(len(here), f, dtype=np.int64))
            pair_l = np.concatenate(pair_c)
            pair_c, pair_f = cap_idx[pair_l], np.concatenate(pair_f)
            if not len(pair_l):
                return
            group_start = torch.zeros(pend["n_images"] + 1, dtype=torch.int32)
            group_start[1:] = torch.from_numpy(np.cumsum(counts).astype(np.int32))
            logits = flt.itm_pairs(pend["y16"], pend["n_images"], ids, lens, group_start=group_start,
                                   max_group=int(counts.max()), pair_text=torch.from_numpy(pair_l), cross=self._cross_of(pend))
        prob = torch.nn.functional.softmax(logits, dim=1)[:, 1].contiguous()
        pend["calls"].append((self._to_host(f"itm{pend.get('tag', '')}{len(pend['calls'])}", prob), pair_c, pair_f))
        pend["n_pairs"] += len(pair_c)

    def _collect(self, pend):
        """Wait for the queued calls and scatter their probabilities into the [captions, F] matrix."""
        for (prob, ev), pair_c, pair_f in pend["calls"]:
            ev.synchronize()
            pend["prob"][pair_c, pair_f] = prob.numpy()
        pend["calls"] = []

    def _filter_enqueue(self, y16, Nv, F, caps_per_video, home=None, tag=""):
        """Queue the filter's text side.  Default: every (frame, caption) pair, as the reference evaluates them, in
        length buckets.  ``itm_short_circuit`` (config, max_filter only): the rule ``max over frames > threshold`` is an
        any(); a generated caption is first scored against the frame it was generated from (``home``), and only the
        captions that did not pass there are scored against the other frames.  Each probability is the one the
        exhaustive schedule computes (a pair's score does not depend on the batch around it), so the kept lists are
        identical; on real captions — which nearly always match their own frame — this is ~1/F of the ITM work."""
        cfg, flt = self.config, self.filterer
        all_caps = [c for caps in caps_per_video for c in caps]
        if not all_caps:
            return None
        ids, lens = flt.tokenize(all_caps)
        lens_np = lens.numpy().astype(np.int64)
        n_caps = np.fromiter((len(c) for c in caps_per_video), dtype=np.int64, count=Nv)
        pend = dict(ids=ids, lens=lens, y16=y16, F=F, n_images=Nv * F, n_pairs=0, calls=[], tag=tag,
                    cap_video=np.repeat(np.arange(Nv, dtype=np.int64), n_caps),
                    prob=np.full((len(all_caps), F), np.nan, dtype=np.float32), short=False)
        every = np.arange(len(all_caps), dtype=np.int64)
        short = (cfg.get("itm_short_circuit", False) and cfg.get("filter_mode", "max_filter") != "avg_filter"
                 and home is not None and F > 1)
        buckets = self._length_buckets(every, lens_np, F)
        # Row-major cross values (cheaper stores) are only readable by the staged attention kernel, i.e. when every call
        # has more than 32 query rows on its busiest image; the short circuit's first phase has one caption per image.
        # The library's rule is per launch: the BUSIEST image of a call has more than 32 rows (its captions in that bucket x the
        # bucket's token cut) -> the smallest such product over the calls decides.
        min_rows = 0
        if not short:
            min_rows = min(min(int(ids.shape[1]), int(lens_np[b].max())) * int(np.bincount(pend["cap_video"][b], minlength=Nv).max())
                           for b in buckets)
        pend["min_rows"] = min_rows
        pend["cross"] = flt.project_image_kv(y16, Nv * F, min_rows)
        if not short:
            for b in buckets:
                self._score(pend, b)
            return pend
        pend["short"] = True
        home_of = np.asarray([home[v].get(c, -1) for v, caps in enumerate(caps_per_video) for c in caps], dtype=np.int64)
        pend["skip"] = home_of
        first = every[home_of >= 0]
        for b in (self._length_buckets(first, lens_np, 1) if len(first) else []):
            self._score(pend, b, frame_of=home_of[b])
        return pend

    def _filter_finish(self, pending, Nv, F, caps_per_video):
        cfg = self.config
        kept = [[] for _ in range(Nv)]
        if pending is None:
            return kept
        thr = cfg["threshold"]
        self._collect(pending)
        prob = pending["prob"]
        if pending["short"]:
            # captions that passed on their home frame are decided; the rest meet the other frames
            with np.errstate(invalid="ignore"):
                passed = np.nan_to_num(prob, nan=-1.0).max(axis=1) > thr
            rest = np.flatnonzero(~passed)
            if len(rest):
                lens_np = pending["lens"].numpy().astype(np.int64)
                for b in self._length_buckets(rest, lens_np, F - 1):
                    self._score(pending, b)
                self._collect(pending)
            keep = np.nan_to_num(prob, nan=-1.0).max(axis=1) > thr
        elif cfg.get("filter_mode", "max_filter") != "avg_filter":
            keep = prob.max(axis=1) > thr         # keep_caption's max rule for every caption at once (no rounding to differ in)
        else:
            keep = np.asarray([keep_caption(prob[c], thr, "avg_filter") for c in range(prob.shape[0])], dtype=bool)
        n = 0
        for v, caps in enumerate(caps_per_video):
            kept[v] = [c for c, k in zip(caps, keep[n:n + len(caps)]) if k]
            n += len(caps)
        return kept


def collect_outputs(items):
    """run_video_CapFilt.py:250-259: (filtered, unfiltered) dicts; videos with no kept caption drop out of the first."""
    filtered, unfiltered = {}, {}
    for item in items:
        if "unfiltered_text" not in item:
            continue
        unfiltered[item["video_id"]] = item["unfiltered_text"]
        if item["text"] != []:
            filtered[item["video_id"]] = item["text"]
    return filtered, unfiltered


def write_outputs(output_dir, filtered, unfiltered):
    """Gather every rank's dicts to rank 0 and write video_text_CapFilt.json / video_text_Cap.json
    (run_video_CapFilt.py:261-291; the tmp-file merge becomes one gather of JSON bytes)."""
    parts = vdist.gather_json([filtered, unfiltered])
    if parts is None:
        return None
    f_all = vdist.merge_rank_dicts([p[0] for p in parts])
    u_all = vdist.merge_rank_dicts([p[1] for p in parts])
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, "video_text_CapFilt.json"), "w") as out:
        json.dump(f_all, out, indent=4)
    with open(os.path.join(output_dir, "video_text_Cap.json"), "w") as out:
        json.dump(u_all, out, indent=4)
    return f_all, u_all
