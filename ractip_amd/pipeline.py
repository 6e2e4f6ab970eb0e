"""Sequences -> joint structure: the probability layer on the GPU (include/ractip_hot.h) followed by RactIP::solve's
integer programme (ractip_amd/ilp.py).  What `ractip s1.fa s2.fa` prints (/root/reference/src/ractip.cpp:1561-1610),
without z-scores and energies.

  python -m ractip_amd.pipeline [--contrafold] [--duplex] [--use-constraint] [--window W [--step S] [--local-hp | --local-hp-both]] [--write-rip FILE] a.fa b.fa

--use-constraint: the structure line that follows each sequence in its FASTA file constrains the folds and the two-molecule
ensemble, as RactIP's -c does (src/ractip.cpp:271-291, 405-447); default path only.
--window W [--step S]: local folding -- bp and up of both molecules are averages over windows of W letters, one every S letters
(Context.local_fold: the quantity RNAplfold defines), for targets too long to fold as a whole; hp comes from the pair as before.
--local-hp (with --window): hp too is a window average -- the longer molecule is windowed and every window hybridized with the whole
shorter one (Context.local_duplex), so nothing is computed over the whole pair.
--local-hp-both (with --window): both molecules are windowed and every window of one is hybridized with every window of the other
(Context.local_duplex2): the route for two long molecules, where not even one of them is folded whole.
--write-rip FILE: also write bp1, bp2, hp as RIP tables (ractip_amd/rip.py) for a stock `ractip --rip FILE --min-w 0`.

  python -m ractip_amd.pipeline --max-span L [--window W [--step S] --local-hp | --local-hp-both] [--duplex] [--write-rip FILE] a.fa b.fa

--max-span L with two files: bp and up[i][w] of both molecules come from span-limited folds (Context.span_fold at the programme's
max_w: one ensemble per molecule, pairs within L letters), hp from the pair as before or, with --window and --local-hp /
--local-hp-both, from the window averages above.  Default (Vienna-BL) model only, no --use-constraint.

  python -m ractip_amd.pipeline --max-span L [--use-constraint] [--threshold T] a.fa

--max-span L: span-limited folding of ONE sequence (Context.span_fold): the McCaskill ensemble of the whole sequence under the
Vienna-BL model with pairs (a, b) only where b - a < L.  Prints ">name logZ <log Z>" and one line "i j p" per pair whose probability
exceeds T (default 0.5), 1-based, row-major, scanned on the device (Context.local_candidates).
--use-constraint (one-file forms only): the structure line that follows the sequence constrains the span fold, translated as for
the whole-sequence folds (fold_constraint); a matched bracket pair must lie within L letters.

  python -m ractip_amd.pipeline --max-span L --all-records [--use-constraint] [--threshold T] many.fa

--all-records: every record of the file is folded, all of them as ONE batch (Context.span_fold_batch), and the lines above are
printed for each record in the file's order.  With --use-constraint every record is folded under its own structure line.

  python -m ractip_amd.pipeline --max-span L --contrafold [--all-records] [--threshold T] one.fa

--contrafold with the one-file forms: the same ensemble and output under the CONTRAfold model (a CONTRAfold context with its span
folds switched on, Context.set_span_contrafold).  The model takes no constraint: with --use-constraint the command exits with a
message.

  python -m ractip_amd.pipeline --contrafold --accessibility [--max-span L [--window W [--step S] --local-hp | --local-hp-both]] a.fa b.fa

--accessibility (two files, with --contrafold): predict(..., accessibility=True) -- the CONTRAfold model's region accessibility
up[i][w], widths 1..max_w, goes into the joint programme.  With --max-span L, bp and up of both molecules come from span folds under
the CONTRAfold model (one batch of two on a context with its span folds and region accessibility switched on), hp from the CONTRAfold
pair path or the window averages.  Without --accessibility, two files with --max-span --contrafold raise as before.
"""
import sys

import math

import numpy as np

from . import energy, hot, ilp, rip, shard


def read_fasta(path):
    name, seq = "", []
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            if seq:
                break
            name = line[1:]
        elif line:
            seq.append(line)
    return name, "".join(seq)


STRUCTURE_CHARS = set("()[].?xle<>|")   # what a FASTA structure line is made of (src/fa.cpp:60-69, plus '<' '>' '|' of fold_constrained)


def read_fasta_with_structure(path):
    """(name, sequence, structure) of the first record: a line after the sequence that consists only of structure characters
    (none of which is a nucleotide code) is the structure line, "" if there is none.  Sequence lines before it are joined as
    read_fasta joins them."""
    name, seq, structure = "", [], ""
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            if seq:
                break
            name = line[1:]
        elif line:
            if seq and set(line) <= STRUCTURE_CHARS:
                structure = line
                break
            seq.append(line)
    return name, "".join(seq), structure


def fold_constraint(structure, n):
    """The structure line of one sequence as RactIP::rnafold hands it to pf_fold (src/ractip.cpp:275-287): '[' ']' 'e' become
    'x', everything else is kept, missing positions are '.'."""
    line = structure[:n]
    return "".join("x" if ch in "[]e" else ch for ch in line) + "." * (n - len(line))


def joint_share(structure, n, first):
    """One molecule's part of joint_constraint: the structure line of s1 (first=True: '[' becomes '(') or of s2 (']' becomes ')');
    '(' ')' 'l' 'x' become 'x', everything else '.', n characters.  What Context.batch_upload_indexed takes per sequence as
    co_first / co_second."""
    forced, to = ("[", "(") if first else ("]", ")")
    line = structure[:n]
    return "".join(to if ch == forced else "x" if ch in "()lx" else "." for ch in line) + "." * (n - len(line))


def joint_constraint(str1, n1, str2, n2):
    """The structure lines of a pair as the default branch of RactIP::rnaduplex hands them to co_pf_fold over s1+s2
    (src/ractip.cpp:409-440): '[' of s1 becomes '(' and ']' of s2 becomes ')', '(' ')' 'l' 'x' become 'x', everything else '.'."""
    return joint_share(str1, n1, True) + joint_share(str2, n2, False)


def probabilities(ctx, s1, s2, structures=None):
    if structures is None:
        ctx.batch_upload([(s1, s2)])
    else:
        str1, str2 = structures
        ctx.batch_upload([(s1, s2)], constraints=[(fold_constraint(str1, len(s1)), fold_constraint(str2, len(s2)))],
                         co_constraints=[joint_constraint(str1, len(s1), str2, len(s2))])
    ctx.batch_compute()
    return ctx.batch_results(0)


def _set_up(ctx, model, opt, duplex, accessibility):
    """the context's settings for one of predict's paths"""
    if model == "vienna":
        ctx.set_max_w(max(1, opt.max_w))
        ctx.set_hybrid(not duplex)
    elif accessibility:
        ctx.set_region_accessibility(True)
        ctx.set_max_w(max(1, opt.max_w))


def local_fold(seq, window, step=1, model="vienna", accessibility=False, device=0, options=None, ctx=None):
    """Window-averaged probabilities of one long sequence: dict(bp_band (n, ld), up (n, max_w), logz, starts) of
    Context.local_fold under predict's settings of model / accessibility / options.max_w."""
    own = ctx is None
    if own:
        ctx = hot.Context(device=device, model=hot.RH_MODEL_VIENNA_BL if model == "vienna" else hot.RH_MODEL_CONTRAFOLD)
    try:
        _set_up(ctx, model, options or ilp.Options(), False, accessibility)
        band, up, logz, starts = ctx.local_fold(seq, window, step)
        return dict(bp_band=band, up=up, logz=logz, starts=starts)
    finally:
        if own:
            ctx.close()


def local_duplex(s1, s2, window, step=1, windowed=2, model="vienna", duplex=False, accessibility=False, device=0, options=None, ctx=None):
    """Window-averaged hybridization of a query on a long target: dict(hp (n1+1, n2+1), logz_pair, starts, bp_band, up, logz) of
    Context.local_duplex under predict's settings of model / duplex / accessibility / options.max_w; bp_band, up and logz are the
    local fold of the windowed molecule, which the same call yields."""
    own = ctx is None
    if own:
        ctx = hot.Context(device=device, model=hot.RH_MODEL_VIENNA_BL if model == "vienna" else hot.RH_MODEL_CONTRAFOLD)
    try:
        _set_up(ctx, model, options or ilp.Options(), duplex, accessibility)
        hp, logz_pair, starts = ctx.local_duplex(s1, s2, window, step, windowed)
        band, up, logz, _ = ctx.local_results()
        return dict(hp=hp, logz_pair=logz_pair, starts=starts, bp_band=band, up=up, logz=logz)
    finally:
        if own:
            ctx.close()


def local_duplex2(s1, s2, window1, step1=1, window2=None, step2=None, model="vienna", duplex=False, device=0, options=None, ctx=None):
    """Window-averaged hybridization of two long molecules, both cut into windows: dict(hp (n1+1, n2+1), logz_pair (nw1, nw2),
    starts1, starts2) of Context.local_duplex2 under predict's settings of model / duplex / options.max_w."""
    own = ctx is None
    if own:
        ctx = hot.Context(device=device, model=hot.RH_MODEL_VIENNA_BL if model == "vienna" else hot.RH_MODEL_CONTRAFOLD)
    try:
        _set_up(ctx, model, options or ilp.Options(), duplex, False)
        hp, logz_pair, starts1, starts2 = ctx.local_duplex2(s1, s2, window1, step1, window2, step2)
        return dict(hp=hp, logz_pair=logz_pair, starts1=starts1, starts2=starts2)
    finally:
        if own:
            ctx.close()


def _predict_local(ctx, s1, s2, model, duplex, opt, default_options, rip_path, accessibility, window, step, local_hp=False, local_hp_both=False):
    """predict with bp and up of both molecules from local folds; hp from the pair path as before, or (local_hp) from local_duplex
    with the longer molecule windowed (s2 on a tie), which also yields that molecule's bp and up, or (local_hp_both) from
    local_duplex2 with both molecules windowed, whose result the local folds behind it leave alone"""
    _set_up(ctx, model, opt, duplex, accessibility)
    bp, up = [None, None], [None, None]
    if local_hp_both:
        hp = ctx.local_duplex2(s1, s2, window, step)[0]
    elif local_hp:
        windowed = 1 if len(s1) > len(s2) else 2
        hp, _, _ = ctx.local_duplex(s1, s2, window, step, windowed)
        band, u, _, _ = ctx.local_results()
        bp[windowed - 1], up[windowed - 1] = hot.band_to_tri(band), u
    else:
        hp = probabilities(ctx, s1, s2)["hp"]   # (fetched before the local folds take the context's batch)
    for k, s in enumerate((s1, s2)):
        if bp[k] is None:
            band, u, _, _ = ctx.local_fold(s, window, step)
            bp[k], up[k] = hot.band_to_tri(band), u
    if rip_path:
        rip.write_rip(rip_path, s1, s2, bp[0], bp[1], hp)
    if model == "vienna" or accessibility:
        return ilp.solve(s1, s2, bp[0], bp[1], hp, up[0], up[1], opt)
    return ilp.solve(s1, s2, bp[0], bp[1], hp, None, None, ilp.Options(min_w=0) if default_options else opt)


def _predict_span(ctx, s1, s2, duplex, opt, rip_path, max_span, window, step, local_hp, local_hp_both, model="vienna"):
    """predict with bp and up of both molecules from span folds at the programme's max_w; hp from the pair path, or from local_duplex
    (the longer molecule windowed, s2 on a tie) / local_duplex2, fetched before the span folds replace the local result.
    model "contrafold": hp from the CONTRAfold pair path (width 1: the span batch brings its own widths), the span folds with the
    context's span folds and region accessibility switched on"""
    if model == "vienna":
        _set_up(ctx, "vienna", opt, duplex, False)
    else:
        ctx.set_span_contrafold(True)
        ctx.set_region_accessibility(True)
    if local_hp_both:
        hp = ctx.local_duplex2(s1, s2, window, step)[0]
    elif local_hp:
        hp = ctx.local_duplex(s1, s2, window, step, 1 if len(s1) > len(s2) else 2)[0]
    else:
        hp = probabilities(ctx, s1, s2)["hp"]
    bp, up = [], []
    for band, u, _ in ctx.span_fold_batch([s1, s2], max_span, max(1, opt.max_w)):   # one batch of two: the bits of two span_fold calls
        bp.append(hot.band_to_tri(band))
        up.append(u)
    if rip_path:
        rip.write_rip(rip_path, s1, s2, bp[0], bp[1], hp)
    return ilp.solve(s1, s2, bp[0], bp[1], hp, up[0], up[1], opt)


def predict(s1, s2, model="vienna", duplex=False, device=0, options=None, ctx=None, rip_path=None, structures=None, accessibility=False,
            window=None, step=1, local_hp=False, local_hp_both=False, max_span=None):
    """model "vienna": RactIP's default path (rnafold + rnaduplex; duplex=True = --duplex, else co_pf_fold), parity
    unpinned; model "contrafold": the --contrafold path (bp from the CONTRAfold engine, width-1 up, accessibility off as
    src/ractip.cpp:1511-1517 demands), hp from the CONTRAfold duplex engine.  structures = (str1, str2): the FASTA structure
    lines, used as constraints (--use-constraint; model "vienna" only).  accessibility=True with model "contrafold" (an extension:
    the reference has no such combination) turns the context's region accessibility on and hands up[i][w], widths 1..options.max_w,
    to the ILP as the default path does.  window=W (and step): bp and up of both molecules are window averages from
    Context.local_fold instead of whole-sequence folds (no structure constraints); with W no shorter than either molecule the
    probabilities, and so the structures, are those of the whole-sequence folds.  local_hp=True (needs window): hp too is a window
    average, from one Context.local_duplex call that windows the longer molecule (s2 on a tie) against the whole shorter one and
    also yields the windowed molecule's bp and up; the other molecule's come from local_fold as before.  local_hp_both=True (needs
    window, excludes local_hp): hp is the window average of Context.local_duplex2 with (window, step) on BOTH molecules -- the route
    for two long molecules, where no whole molecule is folded anywhere; bp and up of both come from local_fold.  max_span=L (model
    "vienna" only, no structure constraints): bp and up[i][w], widths 1..options.max_w, of both molecules come from span-limited
    folds (Context.span_fold: one ensemble of each whole molecule with pairs within L letters) instead; hp comes from the pair path,
    or with window= and local_hp / local_hp_both from the window averages (a window alone has nothing to do here and is refused).
    With L no smaller than either molecule the ensembles, and so the structures, are those of the whole-sequence folds.
    max_span=L with model "contrafold" needs accessibility=True (without it the call raises): hp comes from the CONTRAfold pair path
    (or the window averages), bp and up[i][w] of both molecules from one span batch of two on the context with its span folds and
    region accessibility switched on."""
    if local_hp_both and window is None:
        raise ValueError("local_hp_both needs a window")
    if local_hp_both and local_hp:
        raise ValueError("local_hp_both and local_hp exclude each other")
    if local_hp and window is None:
        raise ValueError("local_hp needs a window")
    if structures is not None and model != "vienna":
        raise ValueError("structure constraints apply to the default (Vienna-BL) path only")
    if structures is not None and window is not None:
        raise ValueError("local folding takes no structure constraints")
    if max_span is not None and model != "vienna" and not accessibility:
        raise ValueError("span-limited folding runs on the default (Vienna-BL) path only, or under the CONTRAfold model with accessibility=True "
                         "(the joint programme takes up[i][w] of the span folds)")
    if max_span is not None and structures is not None:
        raise ValueError("span-limited folding takes no structure constraints")
    if max_span is not None and window is not None and not (local_hp or local_hp_both):
        raise ValueError("max_span with a window needs local_hp or local_hp_both: bp and up come from the span folds")
    own = ctx is None
    if own:
        ctx = hot.Context(device=device, model=hot.RH_MODEL_VIENNA_BL if model == "vienna" else hot.RH_MODEL_CONTRAFOLD)
    try:
        opt = options or ilp.Options()
        if max_span is not None:
            return _predict_span(ctx, s1, s2, duplex, opt, rip_path, max_span, window, step, local_hp, local_hp_both, model)
        if window is not None:
            return _predict_local(ctx, s1, s2, model, duplex, opt, options is None, rip_path, accessibility, window, step, local_hp, local_hp_both)
        if model == "vienna":
            ctx.set_max_w(max(1, opt.max_w))
            ctx.set_hybrid(not duplex)
            r = probabilities(ctx, s1, s2, structures)
            if rip_path:
                rip.write_rip(rip_path, s1, s2, r["bp1"], r["bp2"], r["hp"])
            return ilp.solve(s1, s2, r["bp1"], r["bp2"], r["hp"], r["up1"], r["up2"], opt)
        if accessibility:
            ctx.set_region_accessibility(True)
            ctx.set_max_w(max(1, opt.max_w))
        r = probabilities(ctx, s1, s2)
        if rip_path:
            rip.write_rip(rip_path, s1, s2, r["bp1"], r["bp2"], r["hp"])
        if accessibility:
            return ilp.solve(s1, s2, r["bp1"], r["bp2"], r["hp"], r["up1"].reshape(len(s1), -1), r["up2"].reshape(len(s2), -1), opt)
        if options is None:
            opt = ilp.Options(min_w=0)
        return ilp.solve(s1, s2, r["bp1"], r["bp2"], r["hp"], None, None, opt)
    finally:
        if own:
            ctx.close()


def _span_context(device, model, max_w=1):
    """a context for the span calls: Vienna-BL, or CONTRAfold with its span folds switched on (Context.set_span_contrafold) and, for
    widths above one, its region accessibility (Context.set_region_accessibility)"""
    if model not in ("vienna", "contrafold"):
        raise ValueError("model %r (\"vienna\" or \"contrafold\")" % (model,))
    ctx = hot.Context(device=device, model=hot.RH_MODEL_VIENNA_BL if model == "vienna" else hot.RH_MODEL_CONTRAFOLD)
    if model == "contrafold":
        ctx.set_span_contrafold(True)
        if max_w > 1:
            ctx.set_region_accessibility(True)
    return ctx


def span_fold(seq, max_span, max_w=1, device=0, ctx=None, structure=None, model="vienna"):
    """Span-limited folding of a whole long sequence (Context.span_fold): dict(n, max_span, bp_band (n, min(max_span, n)) with
    bp_band[i, d] = P(i, i + d), up (n, max_w) with up[i, w] = P(letters i .. i + w unpaired), logZ).  ctx: a Vienna-BL context to
    run on (its local result becomes this one; its max_w setting is not used); by default one is made for the call.
    structure: the sequence's FASTA structure line, used as a constraint after the translation of fold_constraint.
    model "contrafold": the same ensemble under the CONTRAfold model (pairs of complementary letters), on a CONTRAfold context with
    its span folds switched on and, for max_w > 1, its region accessibility too; structure= raises ValueError: the model takes no
    constraint.
    predict(max_span=L) runs the joint programme on two of these, without constraints: predict(max_span=, structures=) and the
    two-file --max-span --use-constraint still raise (the open follow-up)."""
    if model == "contrafold" and structure is not None:
        raise ValueError("span-limited folding under the CONTRAfold model takes no structure constraint")
    own = ctx is None
    if own:
        ctx = _span_context(device, model, max_w)
    try:
        band, up, logz = ctx.span_fold(seq, max_span, max_w, None if structure is None else fold_constraint(structure, len(seq)))
        return dict(n=len(seq), max_span=max_span, bp_band=band, up=up, logZ=logz)
    finally:
        if own:
            ctx.close()


def span_fold_batch(seqs, max_span, max_w=1, device=0, ctx=None, structures=None, model="vienna"):
    """span_fold of several long sequences as one batch (Context.span_fold_batch: the item is a dimension of every launch, the
    lengths may differ): a list with the dict of span_fold for every sequence, bit for bit what span_fold gives on the same context.
    ctx: a Vienna-BL context to run on (its local result stays; the batch result becomes this one).
    structures: one FASTA structure line or None per sequence, each used as span_fold uses structure=.
    model "contrafold": as for span_fold; structures= raises ValueError."""
    seqs = list(seqs)
    cons = None
    if model == "contrafold" and structures is not None:
        raise ValueError("span-limited folding under the CONTRAfold model takes no structure constraints")
    if structures is not None:
        if len(structures) != len(seqs):
            raise ValueError("%d structure lines for %d sequences" % (len(structures), len(seqs)))
        cons = [None if t is None else fold_constraint(t, len(s)) for s, t in zip(seqs, structures)]
    own = ctx is None
    if own:
        ctx = _span_context(device, model, max_w)
    try:
        res = ctx.span_fold_batch(seqs, max_span, max_w, cons)
        return [dict(n=len(s), max_span=max_span, bp_band=band, up=up, logZ=logz) for s, (band, up, logz) in zip(seqs, res)]
    finally:
        if own:
            ctx.close()


def read_fasta_records(path):
    """every record of a FASTA file: a list of (name, sequence)"""
    records = []
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            records.append([line[1:], ""])
        elif line and records:
            records[-1][1] += line
    return [(name, seq) for name, seq in records]


def read_fasta_records_with_structure(path):
    """every record of a FASTA file with its structure line: a list of (name, sequence, structure).  Per record the rule of
    read_fasta_with_structure: the first line behind the sequence that consists only of structure characters is the structure
    line ("" if there is none), and the record's lines behind it are not read."""
    records = []
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            records.append([line[1:], "", None])
        elif line and records and records[-1][2] is None:
            if records[-1][1] and set(line) <= STRUCTURE_CHARS:
                records[-1][2] = line
            else:
                records[-1][1] += line
    return [(name, seq, structure or "") for name, seq, structure in records]


def _main_span_records(path, max_span, threshold, use_constraint=False, model="vienna"):
    """--all-records: every record of the file folded as one batch; per record what the one-file form prints"""
    cons = None
    if use_constraint:
        full = read_fasta_records_with_structure(path)
        records = [(name, seq) for name, seq, _ in full]
        cons = [fold_constraint(t, len(seq)) for _, seq, t in full]
    else:
        records = read_fasta_records(path)
    if not records:
        raise SystemExit("%s holds no FASTA record" % path)
    ctx = _span_context(0, model)
    try:
        res = ctx.span_fold_batch([seq for _, seq in records], max_span, 1, cons)
        lists = []
        for k, (_, seq) in enumerate(records):
            rec, total = ctx.span_batch_candidates(k, 0, threshold, cap=max(1, len(seq)))
            if total > len(rec):
                rec, total = ctx.span_batch_candidates(k, 0, threshold, cap=total)
            lists.append(rec.copy())
    finally:
        ctx.close()
    for (name, _), (_, _, logz), rec in zip(records, res, lists):
        print(">%s logZ %.9f" % (name, logz))
        for r in rec:
            print("%d %d %.6g" % (r["i"], r["j"], r["p"]))


def _main_span(argv, max_span):
    threshold = 0.5
    if "--threshold" in argv:
        k = argv.index("--threshold")
        threshold = float(argv[k + 1])
        argv = argv[:k] + argv[k + 2:]
    all_records = "--all-records" in argv
    use_constraint = "--use-constraint" in argv
    model = "contrafold" if "--contrafold" in argv else "vienna"
    argv = [a for a in argv if a not in ("--all-records", "--use-constraint", "--contrafold")]
    files = [a for a in argv if not a.startswith("--")]
    if len(files) != 1 or len(files) != len(argv):
        raise SystemExit("--max-span takes one FASTA file (and --threshold T, --all-records, --use-constraint, --contrafold)")
    if model == "contrafold" and use_constraint:
        raise SystemExit("--max-span --contrafold takes no --use-constraint: the CONTRAfold model takes no structure constraint")
    if all_records:
        return _main_span_records(files[0], max_span, threshold, use_constraint, model)
    if use_constraint:
        name, seq, structure = read_fasta_with_structure(files[0])
    else:
        (name, seq), structure = read_fasta(files[0]), None
    ctx = _span_context(0, model)
    try:
        _, _, logz = ctx.span_fold(seq, max_span, 1, None if structure is None else fold_constraint(structure, len(seq)))
        rec, total = ctx.local_candidates(0, threshold, cap=max(1, len(seq)))   # a letter has at most one pair above 0.5 ...
        if total > len(rec):
            rec, total = ctx.local_candidates(0, threshold, cap=total)            # ... below it the count says how many there are
    finally:
        ctx.close()
    print(">%s logZ %.9f" % (name, logz))
    for r in rec:
        print("%d %d %.6g" % (r["i"], r["j"], r["p"]))


def screen(queries, targets, model="vienna", duplex=False, device=0, options=None, ctx=None, query_structures=None, target_structures=None,
           accessibility=False):
    """The joint structures of the cross product queries x targets from ONE indexed batch: every distinct string is uploaded and
    folded once (hot.index_pairs, Context.batch_upload_indexed), every (query, target) gets its hp.  Returns one list per query
    with predict()'s result for each target; model / duplex / options / accessibility as in predict.
    query_structures / target_structures: one FASTA structure line per query / target ("" for none; a missing side is all ""), used
    as predict uses structures= (--use-constraint; model "vienna" only).  A sequence is then folded once per distinct structure
    line it comes with (hot.index_pairs_structured), and the joint constraints are built on the device from each line's two shares."""
    structured = query_structures is not None or target_structures is not None
    if structured and model != "vienna":
        raise ValueError("structure constraints apply to the default (Vienna-BL) path only")
    pairs = [(q, t) for q in queries for t in targets]
    if not pairs:
        return [[] for _ in queries]
    if structured:
        tq = list(query_structures) if query_structures is not None else [""] * len(queries)
        tt = list(target_structures) if target_structures is not None else [""] * len(targets)
        if len(tq) != len(queries) or len(tt) != len(targets):
            raise ValueError("one structure line per query and per target")
    own = ctx is None
    if own:
        ctx = hot.Context(device=device, model=hot.RH_MODEL_VIENNA_BL if model == "vienna" else hot.RH_MODEL_CONTRAFOLD)
    try:
        with_up = model == "vienna" or accessibility
        opt = options or (ilp.Options() if with_up else ilp.Options(min_w=0))
        if model == "vienna":
            ctx.set_max_w(max(1, opt.max_w))
            ctx.set_hybrid(not duplex)
        elif accessibility:
            ctx.set_region_accessibility(True)
            ctx.set_max_w(max(1, opt.max_w))
        if structured:
            seqs, lines, first, second = hot.index_pairs_structured([((q, a), (t, b)) for q, a in zip(queries, tq) for t, b in zip(targets, tt)])
            ctx.batch_upload_indexed(seqs, list(zip(first, second)),
                                     constraints=[fold_constraint(t, len(s)) for s, t in zip(seqs, lines)],
                                     co_first=[joint_share(t, len(s), True) for s, t in zip(seqs, lines)],
                                     co_second=[joint_share(t, len(s), False) for s, t in zip(seqs, lines)])
        else:
            seqs, first, second = hot.index_pairs(pairs)
            ctx.batch_upload_indexed(seqs, list(zip(first, second)))
        ctx.batch_compute()
        out = []
        for qi in range(len(queries)):
            row = []
            for ti in range(len(targets)):
                (s1, s2), r = pairs[qi * len(targets) + ti], ctx.batch_results(qi * len(targets) + ti)
                up1, up2 = (r["up1"], r["up2"]) if with_up else (None, None)
                if model != "vienna" and with_up:
                    up1, up2 = up1.reshape(len(s1), -1), up2.reshape(len(s2), -1)
                row.append(ilp.solve(s1, s2, r["bp1"], r["bp2"], r["hp"], up1, up2, opt))
            out.append(row)
        return out
    finally:
        if own:
            ctx.close()


def _energies(s1, s2, mats, opt):
    """One iteration of what RactIP::run does with show_energy_/z-score on (src/ractip.cpp:1599-1601, 1645-1650): the joint
    programme with e1, e2, e3 and the two single-sequence programmes with e1s, e2s (all float, like the reference)."""
    r1, r2, _ = ilp.solve(s1, s2, mats["bp1"], mats["bp2"], mats["hp"], mats.get("up1"), mats.get("up2"), opt)
    f32 = np.float32
    e1, e2 = f32(energy.energy_of_structure(s1, r1, noncanonical=True)), f32(energy.energy_of_structure(s2, r2, noncanonical=True))
    e3 = f32(energy.energy_of_duplex(s1, s2, r1, r2))
    r1s, _ = ilp.solve_ss(s1, mats["bp1"], opt)
    r2s, _ = ilp.solve_ss(s2, mats["bp2"], opt)
    e1s, e2s = f32(energy.energy_of_structure(s1, r1s, noncanonical=True)), f32(energy.energy_of_structure(s2, r2s, noncanonical=True))
    return r1, r2, e1, e2, e3, e1s, e2s


def zscore(s1, s2, mode=12, num_shuffling=1000, seed=1, options=None, matrices=None, device=0):
    """The z-score loop of RactIP::run (src/ractip.cpp:1624-1670) on the default path: the native pair and `num_shuffling`
    dinucleotide shuffles (the reference's own RNG order, ractip_amd/shard.py), ALL probability matrices in one device
    pass (modes 1 and 2 shuffle one molecule only: an indexed batch folds the other one once, with the bits it has in every pair), then the programmes and energies per iteration on the host with the reference's float accumulation order.
    `matrices(pairs) -> list of dicts` overrides the probability source (tests)."""
    opt = options or ilp.Options()
    pairs = [(s1, s2)] + shard.zscore_shuffles(s1, s2, mode, num_shuffling, seed)
    if matrices is None:
        ctx = hot.Context(device=device, model=hot.RH_MODEL_VIENNA_BL)
        try:
            ctx.set_max_w(max(1, opt.max_w))
            ctx.set_hybrid(True)
            if mode in (1, 2):
                seqs, first, second = hot.index_pairs(pairs)
                ctx.batch_upload_indexed(seqs, list(zip(first, second)))
                ctx.batch_compute()
                res = ctx.batch_results_all()
                mats = [dict(bp1=res["bp"][i], bp2=res["bp"][j], up1=res["up"][i], up2=res["up"][j], hp=res["hp"][p], logZ=res["logZ"][p])
                        for p, (i, j) in enumerate(zip(first, second))]
            else:
                ctx.batch_upload(pairs)
                ctx.batch_compute()
                mats = ctx.batch_results_all()
        finally:
            ctx.close()
    else:
        mats = matrices(pairs)
    f32 = np.float32
    r1, r2, e1, e2, e3, e1s, e2s = _energies(s1, s2, mats[0], opt)
    tot = f32(f32(e1 + e2) + e3)
    sm = sm2 = sms = sm2s = f32(0.0)
    for (a, b), m in zip(pairs[1:], mats[1:]):
        _, _, ee1, ee2, ee3, ee1s, ee2s = _energies(a, b, m, opt)
        ee = f32(f32(ee1 + ee2) + ee3)
        ees = f32(f32(ee - ee1s) - ee2s)
        sm, sm2 = f32(sm + ee), f32(sm2 + f32(ee * ee))          # src/ractip.cpp:1655-1656
        sms, sm2s = f32(sms + ees), f32(sm2s + f32(ees * ees))
    nsh = f32(num_shuffling)
    mean = f32(sm / nsh); var = max(f32(0.0), f32(f32(sm2 / nsh) - f32(mean * mean)))
    means = f32(sms / nsh); vars_ = max(f32(0.0), f32(f32(sm2s / nsh) - f32(means * means)))
    with np.errstate(divide="ignore", invalid="ignore"):
        z1 = f32(tot - mean) / f32(math.sqrt(var))
        z2 = f32(f32(f32(tot - e1s) - e2s) - means) / f32(math.sqrt(vars_))
    return dict(r1=r1, r2=r2, e1=float(e1), e2=float(e2), e3=float(e3), e1s=float(e1s), e2s=float(e2s), zscore=float(z1), zscore_s=float(z2))


def main(argv):
    rip_path = None
    if "--write-rip" in argv:
        k = argv.index("--write-rip")
        rip_path = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    max_span = None
    if "--max-span" in argv:
        k = argv.index("--max-span")
        max_span, argv = int(argv[k + 1]), argv[:k] + argv[k + 2:]
        valued = {i + 1 for i, a in enumerate(argv) if a in ("--threshold", "--window", "--step")}
        if sum(1 for i, a in enumerate(argv) if not a.startswith("--") and i not in valued) != 2:
            return _main_span(argv, max_span)      # the one-file form
    window, step = None, 1
    for flag in ("--window", "--step"):
        if flag in argv:
            k = argv.index(flag)
            if flag == "--window":
                window = int(argv[k + 1])
            else:
                step = int(argv[k + 1])
            argv = argv[:k] + argv[k + 2:]
    flags = [a for a in argv if a.startswith("--")]
    files = [a for a in argv if not a.startswith("--")]
    if len(files) != 2:
        raise SystemExit(__doc__)
    if "--local-hp" in flags and window is None:
        raise SystemExit("--local-hp requires --window")
    if "--local-hp-both" in flags and window is None:
        raise SystemExit("--local-hp-both requires --window")
    (n1, s1, t1), (n2, s2, t2) = read_fasta_with_structure(files[0]), read_fasta_with_structure(files[1])
    structures = (t1, t2) if "--use-constraint" in flags else None
    r1, r2, _ = predict(s1, s2, model="contrafold" if "--contrafold" in flags else "vienna", duplex="--duplex" in flags, rip_path=rip_path,
                        structures=structures, window=window, step=step, local_hp="--local-hp" in flags,
                        local_hp_both="--local-hp-both" in flags, max_span=max_span, accessibility="--accessibility" in flags)
    print(">%s\n%s\n%s\n>%s\n%s\n%s" % (n1, s1, r1, n2, s2, r2))   # src/ractip.cpp:1607-1610


if __name__ == "__main__":
    main(sys.argv[1:])
