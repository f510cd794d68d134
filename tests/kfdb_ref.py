"""Restatement of the reference's KeyFrameDatabase in plain Python (test infrastructure).

The inverted file is what the reference keeps: one Python list of key frames per word, appended to by add() and walked front
to back by the queries; the order of lKFsSharingWords is whatever that walk produces - nothing here knows about sequence
numbers or sorting.  L1Scoring::score runs on Python floats (IEEE doubles) over the two ascending vectors, the covisibility
tail on numpy float32 scalars like the reference's `float` locals.  Line numbers: src/KeyFrameDatabase.cc and
Thirdparty/DBoW2/DBoW2/ScoringObject.cpp of the reference.
"""
import bisect

import numpy as np

f32 = np.float32


class KF:
    """The members of ORB_SLAM3::KeyFrame the database touches."""

    def __init__(self, kf_id, map_id, word_id, word_val):
        self.mnId, self.map = int(kf_id), int(map_id)
        self.ids = [int(w) for w in word_id]            # mBowVec: a std::map, ascending
        self.vals = [float(v) for v in word_val]
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = 0, 0, f32(0)
        self.mnPlaceRecognitionQuery, self.mnPlaceRecognitionWords, self.mPlaceRecognitionScore = 0, 0, f32(0)
        self.covisible = []                              # GetBestCovisibilityKeyFrames: KF objects, best first
        self.bad = False

    def GetBestCovisibilityKeyFrames(self, n):
        return self.covisible[:n]


def l1_score(ids1, vals1, ids2, vals2):
    """L1Scoring::score (ScoringObject.cpp:23-68); the two lower_bound jumps are bisections of the ascending ids."""
    i, j, n1, n2 = 0, 0, len(ids1), len(ids2)
    score = 0.0
    while i < n1 and j < n2:
        vi, wi = vals1[i], vals2[j]
        if ids1[i] == ids2[j]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif ids1[i] < ids2[j]:
            i = bisect.bisect_left(ids1, ids2[j], i)
        else:
            j = bisect.bisect_left(ids2, ids1[i], j)
    return -score / 2.0


class Database:
    def __init__(self, n_vocab):
        self.n_vocab = n_vocab
        self.inverted = {}                               # mvInvertedFile, sparse: word -> list of KF
        self.kfs = {}                                    # the key frames in the lists
        self.objects = {}                                # every KeyFrame object ever made: erasing one from the database
                                                         # neither destroys it nor takes it out of the covisibility graph

    # :39-45
    def add(self, kf_id, map_id, word_id, word_val):
        kf = self.objects.get(int(kf_id))
        if kf is None:
            kf = self.objects[int(kf_id)] = KF(kf_id, map_id, word_id, word_val)
        else:                                            # the same object comes back, stamps and all
            kf.map, kf.ids, kf.vals = int(map_id), [int(w) for w in word_id], [float(v) for v in word_val]
        self.kfs[kf.mnId] = kf
        for w in kf.ids:
            self.inverted.setdefault(w, []).append(kf)
        return kf

    # :47-66
    def erase(self, kf_id):
        kf = self.kfs.pop(int(kf_id), None)
        if kf is None:
            return
        for w in kf.ids:
            lst = self.inverted.get(w, [])
            for k, other in enumerate(lst):
                if other is kf:
                    del lst[k]
                    break

    # :68-72
    def clear(self):
        self.inverted = {}
        self.kfs = {}

    # :74-98
    def clearMap(self, map_id):
        for w in list(self.inverted):
            self.inverted[w] = [kf for kf in self.inverted[w] if kf.map != map_id]
        self.kfs = {k: kf for k, kf in self.kfs.items() if kf.map != map_id}

    def set_covisibility(self, covis):
        for kf in self.objects.values():
            kf.covisible = [self.objects[k] for k in covis.get(kf.mnId, ()) if k in self.objects]

    # ---- the part both Detect* functions share with the device query: :615-666 resp. :741-787
    def sharing(self, query_id, word_id, word_val, excluded=(), min_words_floor=0, which="place"):
        """Returns dict(kf, words, score, scored, max_common_words, min_common_words) in lKFsSharingWords order and stamps
        the key frames as the reference does."""
        Q, W, S = {"place": ("mnPlaceRecognitionQuery", "mnPlaceRecognitionWords", "mPlaceRecognitionScore"),
                   "reloc": ("mnRelocQuery", "mnRelocWords", "mRelocScore")}[which]
        excluded = set(int(k) for k in excluded)
        ids, vals = [int(w) for w in word_id], [float(v) for v in word_val]
        lKFsSharingWords = []
        for w in ids:
            for pKFi in self.inverted.get(w, []):
                if getattr(pKFi, Q) != query_id:
                    setattr(pKFi, W, 0)
                    if pKFi.mnId not in excluded:
                        setattr(pKFi, Q, query_id)
                        lKFsSharingWords.append(pKFi)
                setattr(pKFi, W, getattr(pKFi, W) + 1)
        maxCommonWords = 0
        for kf in lKFsSharingWords:
            if getattr(kf, W) > maxCommonWords:
                maxCommonWords = getattr(kf, W)
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))      # int * float in float, truncated (:648, :769)
        minCommonWords = max(minCommonWords, int(min_words_floor))
        score, scored = [], []
        for kf in lKFsSharingWords:
            if getattr(kf, W) > minCommonWords:
                si = f32(l1_score(ids, vals, kf.ids, kf.vals))    # float si = mpVoc->score(...)
                setattr(kf, S, si)
                score.append(si)
                scored.append(True)
            else:
                score.append(f32(0))
                scored.append(False)
        return dict(kf=np.array([kf.mnId for kf in lKFsSharingWords], np.int64),
                    words=np.array([getattr(kf, W) for kf in lKFsSharingWords], np.int32),
                    score=np.array(score, np.float32), scored=np.array(scored, bool),
                    max_common_words=maxCommonWords, min_common_words=minCommonWords, _list=lKFsSharingWords)

    # :733-845
    def DetectRelocalizationCandidates(self, frame_id, word_id, word_val, map_id):
        r = self.sharing(frame_id, word_id, word_val, which="reloc")
        lKFsSharingWords = r["_list"]
        if not lKFsSharingWords:
            return []
        lScoreAndMatch = [(kf.mRelocScore, kf) for kf, ok in zip(lKFsSharingWords, r["scored"]) if ok]
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = f32(0)
        for first, pKFi in lScoreAndMatch:
            vpNeighs = pKFi.GetBestCovisibilityKeyFrames(10)
            bestScore = first
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in vpNeighs:
                if pKF2.mnRelocQuery != frame_id:
                    continue
                accScore = f32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpRelocCandidates = []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if pKFi.map != map_id:
                    continue
                if pKFi.mnId not in spAlreadyAddedKF:
                    vpRelocCandidates.append(pKFi.mnId)
                    spAlreadyAddedKF.add(pKFi.mnId)
        return vpRelocCandidates

    # :604-730
    def DetectNBestCandidates(self, kf_id, word_id, word_val, map_id, connected, nNumCandidates, bad_maps=()):
        r = self.sharing(kf_id, word_id, word_val, excluded=connected, which="place")
        lKFsSharingWords = r["_list"]
        if not lKFsSharingWords:
            return [], []
        lScoreAndMatch = [(kf.mPlaceRecognitionScore, kf) for kf, ok in zip(lKFsSharingWords, r["scored"]) if ok]
        if not lScoreAndMatch:
            return [], []
        lAccScoreAndMatch = []
        bestAccScore = f32(0)
        for first, pKFi in lScoreAndMatch:
            vpNeighs = pKFi.GetBestCovisibilityKeyFrames(10)
            bestScore = first
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in vpNeighs:
                if pKF2.mnPlaceRecognitionQuery != kf_id:
                    continue
                accScore = f32(accScore + pKF2.mPlaceRecognitionScore)
                if pKF2.mPlaceRecognitionScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mPlaceRecognitionScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        # lAccScoreAndMatch.sort(compFirst): std::list::sort is stable; insertion keeps equal keys in order
        srt = []
        for item in lAccScoreAndMatch:
            k = len(srt)
            while k > 0 and item[0] > srt[k - 1][0]:
                k -= 1
            srt.insert(k, item)
        vpLoopCand, vpMergeCand = [], []
        spAlreadyAddedKF = set()
        i = 0
        while i < len(srt) and (len(vpLoopCand) < nNumCandidates or len(vpMergeCand) < nNumCandidates):
            pKFi = srt[i][1]
            if pKFi.bad:       # :712 `continue` without advancing spins in the reference; every port has to step on
                i += 1
                continue
            if pKFi.mnId not in spAlreadyAddedKF:
                if map_id == pKFi.map and len(vpLoopCand) < nNumCandidates:
                    vpLoopCand.append(pKFi.mnId)
                elif map_id != pKFi.map and len(vpMergeCand) < nNumCandidates and pKFi.map not in bad_maps:
                    vpMergeCand.append(pKFi.mnId)
                spAlreadyAddedKF.add(pKFi.mnId)
            i += 1
        return vpLoopCand, vpMergeCand
