"""The training CIDEr-D reward on strings, in plain Python: the checker for ``openviic_amd.cider`` (never the thing measured).

What the reference's SCST step computes per generated caption (``trainers/vi_trainer.py:141-147``): document frequencies over a
fixed corpus, tf-idf vectors of the 1..4-grams of the caption and of each reference of its image, a clipped cosine similarity per
n-gram length damped by a Gaussian of the "length" difference, averaged over lengths and references, times 10.  The "length" of a
sentence is its number of bigrams (the reference sums term frequencies where the 0-based n-gram index is 1).
"""
import math
from collections import Counter

ORDERS = 4


def ngram_counts(sentence):
    words = sentence.split()
    return Counter(tuple(words[i:i + n]) for n in range(1, ORDERS + 1) for i in range(len(words) - n + 1))


class CiderOracle:
    def __init__(self, df_corpus, sigma=6.0):
        documents = list(df_corpus.values()) if hasattr(df_corpus, "values") else list(df_corpus)
        self.df = Counter()
        for sentences in documents:
            seen = set()
            for s in sentences:
                seen.update(ngram_counts(s))
            self.df.update(seen)
        self.log_documents = math.log(float(len(documents)))
        self.sigma = sigma

    def vector(self, sentence):
        """(weights {ngram: tf * idf}, norms per n-gram length, number of bigrams)."""
        weights, squares, bigrams = {}, [0.0] * ORDERS, 0
        for gram, tf in ngram_counts(sentence).items():
            w = tf * (self.log_documents - math.log(max(1.0, float(self.df.get(gram, 0)))))
            weights[gram] = w
            squares[len(gram) - 1] += w * w
            bigrams += tf if len(gram) == 2 else 0
        return weights, [math.sqrt(s) for s in squares], bigrams

    def reward(self, hypothesis, references):
        """10 x CIDEr-D of one caption string against the reference strings of its image (float64)."""
        hyp, hyp_norm, hyp_len = self.vector(hypothesis)
        total = [0.0] * ORDERS
        for ref, ref_norm, ref_len in map(self.vector, references):
            sims = [0.0] * ORDERS
            for gram, w in hyp.items():
                r = ref.get(gram, 0.0)
                sims[len(gram) - 1] += min(w, r) * r
            damp = math.exp(-float(hyp_len - ref_len) ** 2 / (2.0 * self.sigma ** 2))
            for n in range(ORDERS):
                if hyp_norm[n] != 0.0 and ref_norm[n] != 0.0:
                    sims[n] /= hyp_norm[n] * ref_norm[n]
                total[n] += sims[n] * damp
        return sum(total) / ORDERS / len(references) * 10.0

    def rewards(self, hypotheses, references):
        """One reward per (caption, its image's reference list)."""
        return [self.reward(h, refs) for h, refs in zip(hypotheses, references)]
