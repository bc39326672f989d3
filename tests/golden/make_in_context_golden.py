"""Generates tests/golden/in_context_prompts_golden.json by running the reference's own
``save_prompt_lines_with_in_context_selection`` (generate_prompts_random_prefix_in_context_selection.py:150-287) on seeded
synthetic inputs.  The module imports ruamel.yaml and sentence_transformers, which this image lacks: ruamel gets an empty stand-in
(never used by the function), ``sentence_transformers`` a stub whose ``SentenceTransformer.encode`` is a fixed function of the
string (tests/sentence_cases.py: stub_vector) and whose ``util.cos_sim`` is the float64 cosine.  The test hands the same stub to
vidil_amd.prompts.in_context_selection_prompt_lines.

usage: python tests/golden/make_in_context_golden.py <directory of the reference checkout>"""
import contextlib
import copy
import io
import json
import os
import sys
import tempfile
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, sys.argv[1])
import sentence_cases as sc  # noqa: E402
from make_prompts_golden import synth  # noqa: E402  (imports the reference's Prompt from the path above)
from visual_token_generation.prompts import Prompt  # noqa: E402


def install_stubs():
    for name in ("ruamel", "ruamel.yaml"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["ruamel"].yaml = sys.modules["ruamel.yaml"]
    st = types.ModuleType("sentence_transformers")
    st.SentenceTransformer = lambda name: sc.StubEncoder()
    st.util = types.SimpleNamespace(cos_sim=lambda a, b: torch.nn.functional.normalize(a.double(), dim=1)
                                    @ torch.nn.functional.normalize(b.double(), dim=1).t())
    sys.modules["sentence_transformers"] = st


def main():
    install_stubs()
    import generate_prompts_random_prefix_in_context_selection as gs

    base = dict(topk=4, visual_token_aggregation_version="v2", prompt_temporal_template="temporal_natural", add_objects=True,
                add_events=False, add_attributes=True, add_scenes=False, add_frame_captions=True, caption_all_video=True)
    long_line = "word " * 60
    runs = []
    for task, target, N, add_asr, caption_all in (("qa", "question", 2, False, True), ("qa", "whole", 3, True, True),
                                                  ("caption", "caption", 2, False, True), ("caption", "caption_asr", 3, True, False),
                                                  ("vlep", "caption", 9, True, True), ("caption", "caption", 1, False, True)):
        # the support set: examples rendered by the reference's Prompt with the ground truth filled in
        sup_cfg = dict(base, prompt_task=task, add_ASR=add_asr, add_original_caption=True, add_answer=True)
        examples = []
        for i in range(6):
            obj = synth(900 + i, 8, 5)
            obj["caption"] = f" support caption {i} "
            fc = {"s": [f"support cap {i} {j}." for j in range(2 + i % 3)]}
            examples.append(Prompt("", seed=3).construct_prompt("s", obj, fc, sup_cfg, f"support question {i}?" if task == "qa" else None,
                                                                f"sa{i}" if task == "qa" else None, f"support line {i}." if add_asr else None))
        vt = {f"v{i}": synth(800 + i, 8, 4) for i in range(6)}
        for i, o in enumerate(vt.values()):
            o["caption"] = [f"gt {i} a", f"gt {i} b", f"gt {i} c"] if i % 2 else f"gt {i}"
        filt = {f"v{i}": [f"cap {i} {j}." for j in range(2 + i)] for i in (0, 1, 3, 5)}
        unf = {f"v{i}": [f"raw {i} {j}" for j in range(5)] for i in (0, 1, 2, 3, 5)}          # v4: no captions at all
        qa = {"v0": [dict(question="q0?", answer="a0")], "v1": [dict(question="q1?", answer="a1"), dict(question="q1b?", answer="a1b")],
              "v2": [dict(question="q2?", answer="a2")], "v5": [dict(question="q5?", answer="a5")]}
        asr = {"v0": ["test hi", "there "], "v1": [], "v2": [" so, ", "what?", long_line, long_line, long_line, long_line, "late"],
               "v3": [""], "v5": [" "]} if add_asr else None
        with tempfile.TemporaryDirectory() as d:
            cfg = dict(base, prompt_task=task, add_ASR=add_asr, add_original_caption=False, add_answer=False, caption_all_video=caption_all,
                       output_path=os.path.join(d, "out_q.jsonl"),
                       request_body=dict(engine="text-davinci-002", prompt="", n=1, temperature=0.0, max_tokens=64, top_p=1,
                                         frequency_penalty=0, presence_penalty=0))
            cfg_in = {k: (dict(v) if isinstance(v, dict) else v) for k, v in cfg.items() if k != "output_path"}
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                gs.save_prompt_lines_with_in_context_selection(copy.deepcopy(vt), filt, unf, N, "INSTRUCTION LINE", list(examples), cfg,
                                                               qa if task == "qa" else None, asr, comparing_target=target)
            lines = open(cfg["output_path"]).read().splitlines()
            idx = json.load(open(os.path.join(d, "out_q__idx_2_videoid.json")))
        runs.append(dict(visual_tokens=vt, filtered=filt, unfiltered=unf, qa=qa if task == "qa" else None, asr=asr, config=cfg_in, N=N,
                         comparing_target=target, examples=examples, lines=lines, idx=idx))
    json.dump(dict(runs=runs), open(os.path.join(HERE, "in_context_prompts_golden.json"), "w"), indent=0)
    print("wrote", len(runs), "in-context-selection runs,", sum(len(r["lines"]) for r in runs), "request lines")


if __name__ == "__main__":
    main()
