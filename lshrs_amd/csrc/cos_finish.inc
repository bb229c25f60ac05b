// cos_finish.inc - the one text of a candidate's end in cosine_kernel (rerank.hip), run by the lane that holds the candidate's
// sums.  Not a translation unit and not a header: statements, #included where they run (the 16-lane finish of the 8-bit rows, the
// lane-0 finish of the others).  Included, not called, for scan_pass.inc's reason: as a function - by value, by reference or as a
// lambda - it moved the register allocation of all twenty instantiations of the kernel, k-loop included; the included text
// compiles to the code the kernel had with these lines written out in it twice.
// The including scope provides: RAGGED; qnorm, scores, status, err; int code (0 a row of the corpus, 2 an index outside it; not 3),
// float d (the dot product), float s2 (||c||^2), int64_t o (where the candidate's score and status go).
// A zero norm turns code 0 into 1; the score is written for code 0, NaN for any other; the code goes to the status byte and -
// RAGGED - into the error bits.
float sc;
if (code == 0) {
  const float cn = sqrtf(s2);
  if (cn == 0.f) code = 1;
  sc = d / (cn * qnorm);
}
if (code != 0) sc = __builtin_nanf("");
scores[o] = sc;
if (status != nullptr) status[o] = (uint8_t)code;
if (RAGGED && code != 0 && err != nullptr) atomicOr(err, code);
